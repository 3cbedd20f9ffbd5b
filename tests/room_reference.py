"""A float64 restatement of the shoebox image-source definition, for the tests of salsa_amd/rooms.py and
salsa_amd/csrc/room_rir.hip.  It shares no code with either: the images are enumerated by six nested loops, and a response is
summed image by image, every image over exactly the taps of its support.  response_of_table is the same sum on the public (7, n)
table of salsa_room_rirs, for tables that no room gives.

    image (n, q): p = (1 - 2 q) o s + 2 n o L,  A = prod_axis b_axis,0^|n - q| b_axis,1^|n| (b^0 = 1),  order = sum_axis |n - q| + |n|
    tap k of receiver rho: d = |p - rho|, tau = d (fs / c) - t0, h[k] += g (A / d) gain_c w(k - tau),
    w(x) = sinc(x) (1 + cos(pi x / H)) / 2 for |x| < H = 16, else 0;  foa: gains (1, u_y, u_z, u_x), u = (p - rho) / d

The float32 YARDSTICK is the same loop with float64 geometry (p, d, tau, the coefficient g A / d gain_c, and k - tau, each rounded to
float32 once) and float32 from the tap argument on: sinc, window, product and the accumulation, image after image.  It is evaluated
in table order and in reversed table order; a comparison takes the larger of the two errors."""
import math

import numpy as np

H = 16
FS, SOUND_SPEED, MIC_RADIUS = 24000, 343.0, 0.042
MIC_DIRECTIONS = ((45, 35), (-45, -35), (135, -35), (-135, 35))


def unit(az_deg, el_deg):
    az, el = math.radians(az_deg), math.radians(el_deg)
    return np.array([math.cos(az) * math.cos(el), math.sin(az) * math.cos(el), math.sin(el)])


def ulp32(x):
    return float(np.spacing(np.float32(x)))


def receivers(audio_format, array):
    array = np.asarray(array, np.float64)
    if audio_format == 'foa':
        return [array]
    return [array + MIC_RADIUS * unit(az, el) for az, el in MIC_DIRECTIONS]


def source(array, direction, distance, align_direct=True, normalize_direct=True, fs=FS, c=SOUND_SPEED):
    """-> (position, t0, g) of a source `distance` metres from the array centre towards direction = (azimuth, elevation)"""
    array = np.asarray(array, np.float64)
    s = array + distance * unit(*direction)
    centre = math.sqrt(float(((s - array) ** 2).sum()))
    t0 = max(0, math.floor(centre * fs / c) - H) if align_direct else 0
    return s, float(t0), centre if normalize_direct else 1.0


def images(size, beta, d_max, max_order=None):
    """every image (n, q, A, order) with A > 0 and order <= max_order in the box |n_axis| <= ceil(d_max / (2 L_axis)) + 1 -- beyond it no
    image is nearer than d_max to any point of the room --, ascending in (n_x, n_y, n_z, q_x, q_y, q_z)"""
    reach = [int(math.ceil(d_max / (2.0 * size[ax]))) + 1 for ax in range(3)]
    out = []
    for nx in range(-reach[0], reach[0] + 1):
        for ny in range(-reach[1], reach[1] + 1):
            for nz in range(-reach[2], reach[2] + 1):
                for qx in (0, 1):
                    for qy in (0, 1):
                        for qz in (0, 1):
                            amp, order = 1.0, 0
                            for ax, (n, q) in enumerate(((nx, qx), (ny, qy), (nz, qz))):
                                low, high = abs(n - q), abs(n)
                                amp *= (beta[2 * ax] ** low if low else 1.0) * (beta[2 * ax + 1] ** high if high else 1.0)
                                order += low + high
                            if amp > 0.0 and (max_order is None or order <= max_order):
                                out.append(((nx, ny, nz), (qx, qy, qz), amp, order))
    return out


def d_max_of(length, t0, fs=FS, c=SOUND_SPEED):
    """no image farther than this reaches a tap below `length`"""
    return (length + H + t0) * c / fs * (1.0 + 1e-9)


def _sum_images(points, src, recs, foa, length, fs_over_c, f32):
    """the one per-image tap code: points yields (p (3,), A) in the order of the sum -> (h (C, length), reached bool (C, length))"""
    _, t0, g = src
    C = 4 if foa else len(recs)
    h = np.zeros((C, length), np.float32 if f32 else np.float64)
    reached = np.zeros((C, length), bool)
    for p, amp in points:
        for m, rho in enumerate(recs):
            v = p - rho
            d = math.sqrt(float(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))
            tau = d * fs_over_c - t0
            k_lo, k_hi = max(0, math.floor(tau - H) + 1), min(length - 1, math.ceil(tau + H) - 1)     # tau - H < k < tau + H
            if k_lo > k_hi:
                continue
            k = np.arange(k_lo, k_hi + 1)
            x = k - tau
            coef = g * amp / d
            gains = [coef, coef * (v[1] / d), coef * (v[2] / d), coef * (v[0] / d)] if foa else [coef]
            if f32:
                x = x.astype(np.float32)
                y = np.float32(np.pi) * x
                with np.errstate(invalid='ignore', divide='ignore'):
                    sinc = np.where(x == 0, np.float32(1), np.sin(y) / y).astype(np.float32)
                w = sinc * (np.float32(0.5) * (np.float32(1) + np.cos(x * np.float32(np.pi / H))))
                w = np.where(np.abs(x) < H, w, np.float32(0)).astype(np.float32)
            else:
                w = np.sinc(x) * 0.5 * (1.0 + np.cos(np.pi * x / H))
            for ch, gc in enumerate(gains):
                row = ch if foa else m
                h[row, k_lo:k_hi + 1] += (np.float32(gc) * w) if f32 else gc * w
                reached[row, k_lo:k_hi + 1] = True
    return h, reached


def response(image_list, size, src, recs, foa, length, f32=False, reverse=False, fs=FS, c=SOUND_SPEED):
    """-> (h (C, length), reached bool (C, length): the taps inside some image's support).  src = (position, t0, g).  f32: the yardstick.
    The delay is d (fs / c) - t0, fs / c one float64 number: what the table-level interface takes."""
    s, L = src[0], np.asarray(size, np.float64)
    points = (((1.0 - 2.0 * np.asarray(q, np.float64)) * s + 2.0 * np.asarray(n, np.float64) * L, amp)
              for n, q, amp, _ in (reversed(image_list) if reverse else image_list))
    return _sum_images(points, src, recs, foa, length, fs / c, f32)


def response_of_table(table, src, recs, foa, length, fs_over_c, f32=False, reverse=False):
    """`response` on the public (7, n) table of salsa_room_rirs (rows: sign x, y, z, shift x, y, z, amplitude): image i lies at
    sign_i o s + shift_i.  The table need not come from a room: the tests of the compaction build theirs by hand."""
    table = np.asarray(table, np.float64)
    assert table.ndim == 2 and table.shape[0] == 7
    s = np.asarray(src[0], np.float64)
    order = range(table.shape[1] - 1, -1, -1) if reverse else range(table.shape[1])
    points = ((table[0:3, i] * s + table[3:6, i], float(table[6, i])) for i in order)
    return _sum_images(points, src, recs, foa, length, fs_over_c, f32)


def table_reference(table, src, recs, foa, length, fs_over_c):
    """-> (ref64, [yardstick in table order, reversed], reached) of a table, each (C, length), read-only: shared, never written"""
    ref, reached = response_of_table(table, src, recs, foa, length, fs_over_c)
    yards = [response_of_table(table, src, recs, foa, length, fs_over_c, f32=True, reverse=rev)[0] for rev in (False, True)]
    for a in [ref, reached] + yards:
        a.setflags(write=False)
    return ref, yards, reached


def reference_and_yardstick(image_list, size, src, recs, foa, length):
    """-> (ref64 (C, length), Y: the larger error of the float32 yardstick in table order and in reversed order, reached)"""
    ref, reached = response(image_list, size, src, recs, foa, length)
    Y = max(float(np.abs(response(image_list, size, src, recs, foa, length, f32=True, reverse=rev)[0].astype(np.float64) - ref).max())
            for rev in (False, True))
    return ref, Y, reached


def bound(ref, Y):
    """the project's rule: max |got - ref64| <= 4 Y + ulp32(max |ref64|)"""
    return 4.0 * Y + ulp32(np.abs(ref).max())
