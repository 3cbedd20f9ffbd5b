"""The moving-source definition of the scene renderer restated in float64, its float32 evaluations (the GPU
tests' yardstick, as in tests/scene_reference.py), and the segment expansion -- all restated here, independently of salsa_amd/scenes.py.

A moving item has trajectory nodes k = 0 .. K - 1 at dry times k S, K = ceil((len - 1) / S) + 1, with responses r_k and windows
w_k(n) = max(0, 1 - |n - k S| / S); it contributes g sum_k (h[r_k, c, :] * (w_k . s))[n - o].  Node k's window is non-zero on the dry
samples ((k - 1) S, (k + 1) S) only, so that is the segment convolved.  `scenes`, `pool`, `bank` are salsa_amd.scenes objects; only
their arrays are read."""
import numpy as np
import scipy.signal

import scene_reference as sr


def n_nodes(length, S):
    return 1 if length <= 1 else (length - 2) // S + 2                         # ceil((length - 1) / S) + 1 without a negative floor


def window64(k, S, length):
    n = np.arange(length, dtype=np.float64)
    return np.maximum(0.0, 1.0 - np.abs(n - k * S) / S)


def expand(scenes, pool, b, n_samples=None):
    """clip b's segments, in rendering order: (event, first dry sample a, one past the last, response, node time k S or None for a
    static item, onset of the ITEM, gain).  A segment whose first sample falls at or past n_samples is left out."""
    S = scenes.traj_step
    for i in range(scenes.clip_start[b], scenes.clip_start[b + 1]):
        e, o, g = int(scenes.event[i]), int(scenes.onset[i]), scenes.gain[i]
        ln = len(pool.signals[e])
        t0, t1 = int(scenes.traj_start[i]), int(scenes.traj_start[i + 1])
        if t1 == t0:
            yield e, 0, ln, int(scenes.rir[i]), None, o, g
            continue
        assert t1 - t0 == n_nodes(ln, S)
        for k in range(t1 - t0):
            a, end = max(0, (k - 1) * S + 1), min(ln, (k + 1) * S)
            if n_samples is None or o + a < n_samples:
                yield e, a, end, int(scenes.traj_rir[t0 + k]), k * S, o, g


def render64_moving(scenes, pool, bank, n_samples, ambient=None):
    """np.convolve per segment and channel, everything float64 (the gain is the float32 value the tables hold)"""
    B, C = scenes.n_clips, bank.n_channels
    S = scenes.traj_step
    out = np.zeros((B, C, n_samples), np.float64) if ambient is None else np.asarray(ambient, np.float64).copy()
    for b in range(B):
        for e, a, end, r, centre, o, g in expand(scenes, pool, b, n_samples):
            s = pool.signals[e].astype(np.float64)[a:end]
            if centre is not None:
                s = s * (1.0 - np.abs(np.arange(a, end, dtype=np.float64) - centre) / S)
            for c in range(C):
                y = np.convolve(bank.rirs[r, c].astype(np.float64), s)[:n_samples - o - a]
                out[b, c, o + a:o + a + len(y)] += float(g) * y
    return out


def render32_moving(scenes, pool, bank, n_samples, ambient=None, block=None):
    """the definition in float32: the window (float)(S - |n - k S|) / (float)S, the windowed sample rounded once, then block=None
    one-shot scipy.signal.fftconvolve (single precision for float32 inputs), else overlap-save at that block size; segments are
    added in float32, in order, then the ambient"""
    B, C = scenes.n_clips, bank.n_channels
    S = scenes.traj_step
    out = np.zeros((B, C, n_samples), np.float32)
    for b in range(B):
        for e, a, end, r, centre, o, g in expand(scenes, pool, b, n_samples):
            s = pool.signals[e][a:end]
            if centre is not None:
                s = s * ((S - np.abs(np.arange(a, end) - centre)).astype(np.float32) / np.float32(S))
            assert s.dtype == np.float32
            for c in range(C):
                h = bank.rirs[r, c]
                y = scipy.signal.fftconvolve(h, s) if block is None else sr._ols32(h, s, block)
                assert y.dtype == np.float32
                y = y[:n_samples - o - a]
                out[b, c, o + a:o + a + len(y)] += np.float32(g) * y
    if ambient is not None:
        out = np.asarray(ambient, np.float32) + out
    return out


def float32_yardstick(scenes, pool, bank, n_samples, ambient, ref64):
    """Y: the largest error of the four float32 evaluations against ref64, and the four of them"""
    errs = [float(np.abs(render32_moving(scenes, pool, bank, n_samples, ambient, blk).astype(np.float64) - ref64).max())
            for blk in sr.EVALUATIONS]
    return max(errs), errs


def support(scenes, pool, bank, n_samples):
    """bool (B, n_samples): the union of the ITEMS' supports [o, o + len + L - 1), which the segments' supports add up to"""
    m = np.zeros((scenes.n_clips, n_samples), bool)
    for b in range(scenes.n_clips):
        for i in range(scenes.clip_start[b], scenes.clip_start[b + 1]):
            o = int(scenes.onset[i])
            m[b, o:o + len(pool.signals[int(scenes.event[i])]) + bank.length - 1] = True
    return m


def frame_node(f, onset, S, K, hop=2400):
    """k(f): the node nearest the centre of label frame f, a tie to the later node"""
    return min(max((2 * (hop * f + hop // 2 - onset) + S) // (2 * S), 0), K - 1)
