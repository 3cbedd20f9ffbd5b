"""Numpy references for the diffuse ambient noise (salsa_amd/ambient.py, salsa_amd/csrc/scene_diffuse.hip),
independent of torch and of the package: the counter hash white(seed, d, n) in unsigned integer arithmetic, the three sums of the
definition with a dtype argument (float64: the reference; float32, in natural or reversed order: the yardstick the GPU bounds are formed
from, as tests/attn_reference.py does it), the expected power per channel, and a dense quadrature of the sphere for ideal coherences.

    mix64(z):  z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31        (mod 2^64)
    h = mix64(mix64(seed + G) + ((d << 48) | (n + 1024)) G),   G = 0x9E3779B97F4A7C15,   n >= -1024, d < 256
    white = float32(u_0 + u_1 + u_2 + u_3 - 131070) float32(sqrt(3 / (2^32 - 1))),   u_i = (h >> 16 i) & 0xFFFF"""
import numpy as np

WHITE_LEAD = 1024
WHITE_SCALE = np.float32(np.sqrt(3.0 / (65536.0 ** 2 - 1.0)))
_G, _M1, _M2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def mix64(z):
    z = np.asarray(z, np.uint64)
    with np.errstate(over='ignore'):
        z = z ^ (z >> np.uint64(30))
        z = z * _M1
        z = z ^ (z >> np.uint64(27))
        z = z * _M2
        return z ^ (z >> np.uint64(31))


def white_fields(seed, d, n):
    """the four 16-bit fields, int64 (..., 4), for a seed (any integer, taken mod 2^64), a direction d and samples n (an int64 array)"""
    n = np.asarray(n, np.int64)
    if np.any(n < -WHITE_LEAD) or not 0 <= int(d) < 256:
        raise ValueError('white is defined for n >= -%d and 0 <= d < 256' % WHITE_LEAD)
    with np.errstate(over='ignore'):
        key = mix64(np.array(int(seed) % (1 << 64), np.uint64) + _G)
        idx = (np.uint64(int(d)) << np.uint64(48)) | (n + WHITE_LEAD).astype(np.uint64)
        h = mix64(key + idx * _G)
    return np.stack([(h >> np.uint64(s)) & np.uint64(0xFFFF) for s in (0, 16, 32, 48)], axis=-1).astype(np.int64)


def white(seed, d, n):
    """float32, exact to the bit: the integer is below 2^24 and the product rounds once"""
    return (white_fields(seed, d, n).sum(axis=-1) - 131070).astype(np.float32) * WHITE_SCALE


def diffuse(mix, colour, seed, scale, n_samples, inp=None, dtype=np.float64, reverse=False):
    """out (C, n_samples) of ONE clip: mix (D, C, La), colour (Lg,), scale a number, inp (C, n_samples) or None.  Every operand is cast to
    dtype first and every sum accumulates in it, term by term: d outer, k inner, then j, ascending -- or all three descending with
    reverse=True."""
    mix, colour = np.asarray(mix, dtype), np.asarray(colour, dtype)
    D, Cn, La = mix.shape
    Lg, N = len(colour), int(n_samples)
    T, t0 = N + Lg - 1, -(Lg - 1)                                             # m on the samples t0 .. N - 1
    order = (lambda r: reversed(range(r))) if reverse else range
    m = np.zeros((Cn, T), dtype)
    for d in order(D):
        w = white(seed, d, np.arange(t0 - (La - 1), N, dtype=np.int64)).astype(dtype)      # w[i] is sample t0 - (La - 1) + i
        for k in order(La):
            m += mix[d, :, k:k + 1] * w[None, La - 1 - k:La - 1 - k + T]
    y = np.zeros((Cn, N), dtype)
    for j in order(Lg):
        y += colour[j] * m[:, Lg - 1 - j:Lg - 1 - j + N]
    out = dtype(scale) * y
    return out if inp is None else out + np.asarray(inp, dtype)


def channel_power(mix, colour):
    """P_c = sum_d sum_n (sum_k mix[d][c][k] colour[n - k])^2, float64 (C,): the expected mean square per channel at scale 1"""
    mix, colour = np.asarray(mix, np.float64), np.asarray(colour, np.float64)
    D, Cn, La = mix.shape
    full = np.zeros((D, Cn, La + len(colour) - 1))
    for k in range(La):
        full[:, :, k:k + len(colour)] += mix[:, :, k:k + 1] * colour
    return (full ** 2).sum(axis=(0, 2))


def dense_sphere(n_polar=64, n_azimuth=128):
    """A quadrature of the sphere with n_polar x n_azimuth >= 4096 points: Gauss-Legendre nodes in cos(polar angle), equal steps in azimuth.
    -> unit vectors (Q, 3) as (x, y, z), weights (Q,) that sum to one.  Exact for spherical polynomials of degree < min(2 n_polar,
    n_azimuth)."""
    z, wz = np.polynomial.legendre.leggauss(n_polar)
    phi = (np.arange(n_azimuth) + 0.5) * (2.0 * np.pi / n_azimuth)
    r = np.sqrt(1.0 - z * z)
    u = np.stack([np.outer(r, np.cos(phi)), np.outer(r, np.sin(phi)), np.outer(z, np.ones(n_azimuth))], axis=-1).reshape(-1, 3)
    w = np.outer(wz, np.ones(n_azimuth)).reshape(-1)
    assert len(u) >= 4096
    return u, w / w.sum()


def coherence(transfer, weights=None):
    """transfer complex (F, Q, C): channel c's response to a plane wave from point q at frequency f.  -> the coherence matrix (F, C, C) of
    the field the weighted points make, sum_q w_q T_qi conj(T_qj) over the root of the two powers, and the powers (F, C)."""
    T = np.asarray(transfer, np.complex128)
    w = np.full(T.shape[1], 1.0 / T.shape[1]) if weights is None else np.asarray(weights, np.float64)
    S = np.einsum('q,fqi,fqj->fij', w, T, np.conj(T))
    p = np.real(np.einsum('fii->fi', S))
    return S / np.sqrt(p[:, :, None] * p[:, None, :]), p


def foa_transfer(u, n_freqs=1):
    """the FOA gains (W, Y, Z, X) = (1, u_y, u_z, u_x), the same at every frequency"""
    g = np.stack([np.ones(len(u)), u[:, 1], u[:, 2], u[:, 0]], axis=-1).astype(np.complex128)
    return np.broadcast_to(g, (n_freqs,) + g.shape)


def open_transfer(u, capsules, freqs, c):
    """open capsules at the points `capsules` (M, 3) metres: a plane wave from u reaches capsule m earlier by p_m . u / c"""
    return np.exp(2j * np.pi * np.asarray(freqs, np.float64)[:, None, None] * (u @ np.asarray(capsules).T)[None] / c)
