"""A float64 restatement of the octave-band rooms for the tests of salsa_amd/rooms.py and
salsa_amd/csrc/room_bands.hip.  It shares no code with either; the image sums are room_reference's.

    filters     e_b = f_b sqrt(2); low_b(f) = 1 for f <= e_b 2^(-1/4), 0 for f >= e_b 2^(1/4), else cos^2(pi (log2(f / e_b) + 1/4)); G_0 = low_0,
                G_b = low_b - low_(b-1), G_(K-1) = 1 - low_(K-2); h_b[n] = w[n] / N sum_m c_m G_b(m fs / N) cos(2 pi m (n - D) / N), N = 8192,
                c_0 = c_(N/2) = 1, else 2 -- the inverse real FFT written as a cosine sum --, w = np.hanning(2 D + 3)[1:-1]
    band rows   r_b on the taps first .. first + n - 1 of a (6 + K, n) table: room_reference.response_of_table on the 7-row table of band b
                with the time origin moved by `first`
    merge       out[k] = sum_b sum_j h_b[j] r_b[k + 2 D - j] (r_b indexed from its first tap -D);  split  y_b[k] = sum_j h_b[j] x[k + D - j]

The float32 YARDSTICK of a filter sum is the chain acc <- fl(acc + fl(h x)), products and sums each rounded to float32, in the
definition's order (b ascending, j ascending) and in the reversed order; a comparison takes the larger of the two errors.  The
yardstick of a band row is room_reference's."""
import numpy as np

import room_reference as rr

NFFT = 8192
OCTAVE_BANDS = (125, 250, 500, 1000, 2000, 4000, 8000)


def low_pass(f, edge):
    f = np.asarray(f, np.float64)
    out = np.ones_like(f)
    pos = f > 0
    u = np.log2(f[pos] / edge)
    out[pos] = np.where(u <= -0.25, 1.0, np.where(u >= 0.25, 0.0, np.cos(np.pi * (np.clip(u, -0.25, 0.25) + 0.25)) ** 2))
    return out


def gains(f, bands):
    """G (K, len(f)) at the frequencies f"""
    K = len(bands)
    if K == 1:
        return np.ones((1, len(f)))
    low = [low_pass(f, b * np.sqrt(2.0)) for b in bands[:-1]]
    return np.stack([low[0]] + [low[b] - low[b - 1] for b in range(1, K - 1)] + [1.0 - low[K - 2]])


def filters(fs, bands=OCTAVE_BANDS, half=1024):
    """(K, 2 half + 1) float64 by the cosine sum"""
    m = np.arange(NFFT // 2 + 1)
    G = gains(m * (float(fs) / NFFT), bands)
    c = np.full(len(m), 2.0)
    c[0] = c[-1] = 1.0
    n = np.arange(-half, half + 1)
    basis = np.cos((2.0 * np.pi / NFFT) * ((m[:, None] * n[None]) % NFFT))      # (the product reduced mod N as whole numbers: exact)
    return ((G * c[None]) @ basis) / NFFT * np.hanning(2 * half + 3)[1:-1][None]


def band_rows(table, src, recs, foa, first, n_taps, fs_over_c, bands=None):
    """-> (ref64 (C, K, n_taps), [yardstick in table order, reversed] float32, reached bool) of a (6 + K, n) table on the taps first ..."""
    table = np.asarray(table, np.float64)
    K = table.shape[0] - 6
    moved = (src[0], src[1] + first, src[2])                                   # tau - first: tap first becomes index 0
    parts = [rr.table_reference(np.concatenate([table[:6], table[6 + b:7 + b]]), moved, recs, foa, n_taps, fs_over_c)
             for b in (range(K) if bands is None else bands)]
    ref = np.stack([p[0] for p in parts], axis=1)
    yards = [np.stack([p[1][i] for p in parts], axis=1) for i in (0, 1)]
    reached = np.stack([p[2] for p in parts], axis=1)
    for a in [ref, reached] + yards:
        a.setflags(write=False)
    return ref, yards, reached


def _chain32(h, cols, reverse):
    """h (T,) float32 taps, cols(t) -> the float32 inputs (..., L) that tap t multiplies; the chain in order, or reversed"""
    order = range(len(h) - 1, -1, -1) if reverse else range(len(h))
    acc = None
    for t in order:
        term = (h[t] * cols(t)).astype(np.float32)
        acc = term if acc is None else (acc + term).astype(np.float32)
    return acc


def merge(r, h, f32=False, reverse=False):
    """r (n, K, L + 2 D), h (K, 2 D + 1) -> (n, L): float64, or the float32 yardstick chain"""
    n, K, ext = r.shape
    T = h.shape[1]
    L = ext - (T - 1)
    if not f32:
        out = np.zeros((n, L))
        for b in range(K):
            for j in range(T):
                out += float(h[b, j]) * r[:, b, T - 1 - j:T - 1 - j + L].astype(np.float64)
        return out
    flat = h.astype(np.float32).reshape(-1)
    r = r.astype(np.float32)
    return _chain32(flat, lambda t: r[:, t // T, T - 1 - t % T:T - 1 - t % T + L], reverse)


def split(x, h, f32=False, reverse=False):
    """x (n, L), h (K, 2 D + 1) -> (n, K, L)"""
    n, L = x.shape
    K, T = h.shape
    D = (T - 1) // 2
    xe = np.zeros((n, L + 2 * D), np.float32 if f32 else np.float64)
    xe[:, D:D + L] = x
    if not f32:
        out = np.zeros((n, K, L))
        for b in range(K):
            for j in range(T):
                out[:, b] += float(h[b, j]) * xe[:, T - 1 - j:T - 1 - j + L]
        return out
    h = h.astype(np.float32)
    return np.stack([_chain32(h[b], lambda t: xe[:, T - 1 - t:T - 1 - t + L], reverse) for b in range(K)], axis=1)


def yard_error(ref, yards):
    return max(float(np.abs(y.astype(np.float64) - ref).max()) for y in yards)


def bound(ref, Y, factor=4.0):
    """the project's rule: max |got - ref64| <= 4 Y + ulp32(max |ref64|)"""
    return factor * Y + rr.ulp32(np.abs(ref).max())


def room_response(size, beta, bands, half, fs, src, recs, foa, length, max_order=None, c=rr.SOUND_SPEED):
    """The banded response of a room, beta (K, 6) -> (ref64 (C, length), yards [2] float32 (C, length)): the images by room_reference's six
    loops with any band's beta > 0 (an image is kept iff some band carries it), the band rows on the taps -half .. length + half - 1, the
    float32 filters (the definition's: octave filters rounded once), merged in float64; the yardstick merges float32 rows in float32."""
    beta = np.asarray(beta, np.float64)
    K = len(beta)
    d_max = rr.d_max_of(length + half, src[1], fs, c)
    lists = [{(n, q): amp for n, q, amp, _ in rr.images(size, beta[b], d_max, max_order)} for b in range(K)]
    keys = sorted(set().union(*lists))                                         # ascending (n, q): the canonical order
    L = np.asarray(size, np.float64)
    table = np.array([list(1.0 - 2.0 * np.array(q)) + list(2.0 * np.array(n) * L) + [lists[b].get((n, q), 0.0) for b in range(K)]
                      for n, q in keys]).T
    ref, yards, _ = band_rows(table, src, recs, foa, -half, length + 2 * half, fs / c)
    h = filters(fs, bands, half).astype(np.float32)
    return merge(ref, h), [merge(y, h, f32=True, reverse=rev) for y, rev in zip(yards, (False, True))], table
