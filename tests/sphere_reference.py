"""A float64 restatement of the rigid-sphere capsule model, for the tests of salsa_amd/rooms.py (baffle='rigid') and
salsa_amd/csrc/room_sphere.hip.  It shares no code with either.

    series       H(f, Theta) = sum_{n=0}^{N} i^n (2 n + 1) b_n(k R) P_n(cos Theta),  b_n(x) = j_n(x) - j_n'(x) / h_n^(2)'(x) h_n^(2)(x), in
                 THAT form (the module evaluates the Wronskian form), the derivatives by f_n' = f_{n-1} - (n + 1) / x f_n and P_n by
                 Bonnet's recurrence; only j_n and y_n themselves come from scipy.
    sphere filter a_Theta[n] = irfft(H(f_l, Theta) T(f_l), NFFT)[n mod NFFT]; T = 1 up to 0.75 Nyquist, a raised cosine to 0 at Nyquist.
    weight       h_Theta(x) = sum_{n=-NA}^{NB-1} a_Theta[n] w(x - n), w the Hann-windowed sinc of half width H = 16: zero outside (-LEAD,
                 TRAIL), LEAD = NA + 16, TRAIL = NB + 15.  h_full sums over ALL NFFT taps: what the support cuts off.
    table        S[q][p][j] = h_{q pi / Q}(j - (LEAD - 1) - p / P), rounded to float32 once.
    definition   weight of tap k of an image at delay tau and angle Theta: with k0 = floor tau, fr = tau - k0, j = k - k0 + LEAD - 1, qf =
                 Theta Q / pi, q = min(floor qf, Q - 1), wq = qf - q, pf = fr P, p = min(floor pf, P - 1), wp = pf - p:
                 (1 - wq) ((1 - wp) S[q][p][j] + wp S[q][p+1][j]) + wq ((1 - wp) S[q+1][p][j] + wp S[q+1][p+1][j]),  0 <= j < LEAD + TRAIL
    response     out[m, k] += g (A / d) weight, d and tau to the array CENTRE, cos Theta_m = clamp(v . unit_m / d), v the image's offset.

The float32 YARDSTICK is the same per-image loop with the float64 geometry (k0, wq, wp and the coefficient each rounded to float32 once)
and float32 from the table lookup on, in table order and in reversed table order."""
import math

import numpy as np

from room_reference import bound, ulp32  # noqa: F401  (the project's rule: 4 Y + ulp32(max |ref|))

H = 16
FS, SOUND_SPEED, MIC_RADIUS = 24000, 343.0, 0.042
MIC_DIRECTIONS = ((45, 35), (-45, -35), (135, -35), (-135, 35))
ORDER, NFFT = 48, 1024
Q, P, NA, NB = 180, 32, 16, 32
LEAD, TRAIL = NA + H, NB + H - 1
LT = LEAD + TRAIL


def unit(az_deg, el_deg):
    az, el = math.radians(az_deg), math.radians(el_deg)
    return np.array([math.cos(az) * math.cos(el), math.sin(az) * math.cos(el), math.sin(el)])


def capsule_units():
    return np.stack([unit(az, el) for az, el in MIC_DIRECTIONS])


def series(f, cos_theta, radius=MIC_RADIUS, c=SOUND_SPEED, order=ORDER):
    """H(f, Theta) for arrays broadcast against each other, complex128"""
    from scipy.special import spherical_jn, spherical_yn
    f, ct = np.asarray(f, np.float64), np.asarray(cos_theta, np.float64)       # (the Bessel functions on f's own shape, not the broadcast one)
    x = 2.0 * np.pi * f / c * radius
    zero = x == 0
    x = np.where(zero, 1.0, x)
    total = np.zeros(np.broadcast(f, ct).shape, np.complex128)
    p_prev, p_cur = np.zeros_like(ct), np.ones_like(ct)                        # P_{-1} (unused), P_0
    j_prev = y_prev = None
    for n in range(order + 1):
        jn, yn = spherical_jn(n, x), spherical_yn(n, x)
        j1, y1 = spherical_jn(n + 1, x), spherical_yn(n + 1, x)
        if n == 0:
            djn, dyn = -j1, -y1
        else:
            djn, dyn = j_prev - (n + 1) / x * jn, y_prev - (n + 1) / x * yn
        h2, dh2 = jn - 1j * yn, djn - 1j * dyn
        b = jn - djn / dh2 * h2
        total += (1j ** n) * (2 * n + 1) * b * p_cur
        p_prev, p_cur = p_cur, ((2 * n + 1) * ct * p_cur - n * p_prev) / (n + 1)
        j_prev, y_prev = jn, yn
    return np.where(zero, 1.0 + 0.0j, total)


def taper(f, fs=FS):
    f0, f1 = 0.75 * 0.5 * fs, 0.5 * fs
    return np.where(f <= f0, 1.0, np.where(f >= f1, 0.0, 0.5 * (1.0 + np.cos(np.pi * (f - f0) / (f1 - f0)))))


def sphere_filter(theta, fs=FS):
    """a_Theta over one period, (..., NFFT): index n mod NFFT"""
    f = np.arange(NFFT // 2 + 1) * (fs / NFFT)
    return np.fft.irfft(series(f, np.cos(np.asarray(theta, np.float64))[..., None]) * taper(f, fs), NFFT, axis=-1)


def w(x):
    x = np.asarray(x, np.float64)
    return np.where(np.abs(x) < H, np.sinc(x) * 0.5 * (1.0 + np.cos(np.pi * x / H)), 0.0)


def h_cut(theta, x, a=None):
    """h_Theta(x) of the definition: the filter cut to [-NA, NB).  theta (T,), x (X,) -> (T, X); a: sphere_filter(theta), if at hand"""
    a = sphere_filter(theta) if a is None else a
    taps = np.arange(-NA, NB)
    return a[:, taps % NFFT] @ w(np.asarray(x, np.float64)[None, :] - taps[:, None])


def h_full(theta, x, a=None):
    """the same sum over the whole period n in [-NFFT / 2, NFFT / 2): what the band-limited series gives before the support is cut"""
    a = sphere_filter(theta) if a is None else a
    taps = np.arange(-NFFT // 2, NFFT // 2)
    return a[:, taps % NFFT] @ w(np.asarray(x, np.float64)[None, :] - taps[:, None])


def table():
    """S float32 (Q + 1, P + 1, LT), evaluated entry by entry from the definition (row P computed, not copied)"""
    theta = np.arange(Q + 1) * np.pi / Q
    a = sphere_filter(theta)
    out = np.empty((Q + 1, P + 1, LT))
    for p in range(P + 1):
        out[:, p, :] = h_cut(theta, np.arange(LT) - (LEAD - 1) - p / P, a)
    return out.astype(np.float32)


def cell(theta, fr, nq, npp):
    """-> (q, wq, p, wp): the table cell of angle theta and fraction fr and the two weights, with the definition's clamps"""
    qf, pf = theta * (nq / math.pi), fr * npp
    q, p = min(max(int(math.floor(qf)), 0), nq - 1), min(max(int(math.floor(pf)), 0), npp - 1)
    return q, qf - q, p, pf - p


def interp(S, theta, fr):
    """the definition's bilinear weight of all taps j = 0 .. lead + trail - 1 at angle theta and fraction fr, float64 (LT,)"""
    q, wq, p, wp = cell(theta, fr, S.shape[0] - 1, S.shape[1] - 1)
    s00, s01, s10, s11 = (S[a, b].astype(np.float64) for a, b in ((q, p), (q, p + 1), (q + 1, p), (q + 1, p + 1)))
    return (1.0 - wq) * ((1.0 - wp) * s00 + wp * s01) + wq * ((1.0 - wp) * s10 + wp * s11)


def response_of_table(images, src, centre, units, S, lead, trail, length, fs_over_c, f32=False, reverse=False):
    """The per-image loop on the public (7, n) image table (rows: sign x, y, z, shift x, y, z, amplitude) and a sphere table S float32
    (Q + 1, P + 1, lead + trail).  src = (position, t0, g) -> (h (4, length), reached bool (4, length): the taps inside some image's
    lead + trail taps).  f32: the yardstick."""
    images = np.asarray(images, np.float64)
    assert images.ndim == 2 and images.shape[0] == 7 and S.shape[2] == lead + trail and S.dtype == np.float32
    s, t0, g = np.asarray(src[0], np.float64), float(src[1]), float(src[2])
    centre, units = np.asarray(centre, np.float64), np.asarray(units, np.float64)
    nq, npp = S.shape[0] - 1, S.shape[1] - 1
    h = np.zeros((4, length), np.float32 if f32 else np.float64)
    reached = np.zeros((4, length), bool)
    order = range(images.shape[1] - 1, -1, -1) if reverse else range(images.shape[1])
    one = np.float32(1)
    for i in order:
        v = images[0:3, i] * s + images[3:6, i] - centre
        d = math.sqrt(float(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))
        tau = d * fs_over_c - t0
        k0 = math.floor(tau)
        fr = tau - k0
        j_lo, j_hi = max(0, lead - 1 - k0), min(lead + trail - 1, length - 1 - k0 + lead - 1)       # 0 <= k = k0 + j - (lead - 1) < length
        if j_lo > j_hi:
            continue
        k_lo, k_hi = k0 + j_lo - (lead - 1), k0 + j_hi - (lead - 1)
        coef = g * float(images[6, i]) / d
        for m in range(4):
            cos = min(1.0, max(-1.0, float(v[0] * units[m, 0] + v[1] * units[m, 1] + v[2] * units[m, 2]) / d))
            theta = math.acos(cos)
            if f32:
                q, wq, p, wp = cell(theta, fr, nq, npp)
                wq, wp = np.float32(wq), np.float32(wp)
                e0 = (one - wp) * S[q, p, j_lo:j_hi + 1] + wp * S[q, p + 1, j_lo:j_hi + 1]
                e1 = (one - wp) * S[q + 1, p, j_lo:j_hi + 1] + wp * S[q + 1, p + 1, j_lo:j_hi + 1]
                h[m, k_lo:k_hi + 1] += np.float32(coef) * ((one - wq) * e0 + wq * e1)
            else:
                h[m, k_lo:k_hi + 1] += coef * interp(S, theta, fr)[j_lo:j_hi + 1]
            reached[m, k_lo:k_hi + 1] = True
    return h, reached


def table_reference(images, src, centre, units, S, lead, trail, length, fs_over_c):
    """-> (ref64, Y: the larger error of the yardstick in table order and in reversed order, reached), the arrays read-only"""
    ref, reached = response_of_table(images, src, centre, units, S, lead, trail, length, fs_over_c)
    Y = max(float(np.abs(response_of_table(images, src, centre, units, S, lead, trail, length, fs_over_c, f32=True, reverse=rev)[0].astype(np.float64)
                         - ref).max()) for rev in (False, True))
    ref.setflags(write=False)
    reached.setflags(write=False)
    return ref, Y, reached


def room_image_table(size, beta, d_max):
    """the (7, n) table of a room from room_reference's own enumeration, in its canonical order"""
    import room_reference as rr
    imgs = rr.images(size, beta, d_max)
    L = np.asarray(size, np.float64)
    cols = [np.concatenate([1.0 - 2.0 * np.asarray(q, np.float64), 2.0 * np.asarray(n, np.float64) * L, [amp]]) for n, q, amp, _ in imgs]
    return np.ascontiguousarray(np.stack(cols, axis=1))


def source(array, direction, distance, align_direct=True, normalize_direct=True, fs=FS, c=SOUND_SPEED):
    """-> (position, t0, g): room_reference.source with LEAD for H"""
    array = np.asarray(array, np.float64)
    s = array + distance * unit(*direction)
    centre = math.sqrt(float(((s - array) ** 2).sum()))
    t0 = max(0, math.floor(centre * fs / c) - LEAD) if align_direct else 0
    return s, float(t0), centre if normalize_direct else 1.0


def d_max_of(length, t0, fs=FS, c=SOUND_SPEED):
    return (length + LEAD + t0) * c / fs * (1.0 + 1e-9)
