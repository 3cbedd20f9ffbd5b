"""Numpy / float64 restatements of the Multi-ACCDOA rules and the input builders of tests/test_multi_accdoa_*.py.
Written from the rules, not from the product: nothing of salsa_amd is imported.  Layout everywhere: C real classes, pseudo-class
p = n * C + c for track / slot n; sed (rows, 3 C); doa (rows, 9 C) = [x | y | z] blocks of 3 C columns."""
import math

import numpy as np

# candidate assignments (track 0, 1, 2 -> source) by the number of active slots, in index order; -1: the zero target
CANDIDATES = {
    0: [(-1, -1, -1)],
    1: [(0, 0, 0)],
    2: [(0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0)],
    3: [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)],
}


def to_items(a, C):
    """(rows, 9 C) -> (rows, C, track, axis)"""
    return a.reshape(a.shape[0], 3, 3, C).transpose(0, 3, 2, 1)


def from_items(a):
    """(rows, C, track, axis) -> (rows, 9 C)"""
    return np.ascontiguousarray(a.transpose(0, 3, 2, 1)).reshape(a.shape[0], -1)


# ------------------------------------------------------------------------------------------------------------------ ADPIT loss
def adpit_reference(doa, sed_gt, doa_gt, C):
    """-> dict: chosen (rows, C) uint8, item (rows, C) float64 = e_min / 9, g_doa (rows, 9 C) float32, loss = the exactly rounded
    sum of the items / (rows C) as a Python float (math.fsum; NaN when an item is not finite), k (rows, C) the active slots."""
    doa, sed_gt, doa_gt = np.asarray(doa, np.float32), np.asarray(sed_gt, np.float32), np.asarray(doa_gt, np.float32)
    rows = doa.shape[0]
    P, T = to_items(doa, C).astype(np.float64), to_items(doa_gt, C).astype(np.float64)
    s = sed_gt.reshape(rows, 3, C).transpose(0, 2, 1) > np.float32(0.5)                # (rows, C, slot)
    k = s.sum(-1)
    order = np.argsort(~s, axis=-1, kind='stable')                                     # the active slots first, in slot order
    S = np.take_along_axis(T, order[..., None], axis=2)
    chosen = np.zeros((rows, C), np.uint8)
    e_min = np.zeros((rows, C), np.float64)
    t_chosen = np.zeros((rows, C, 3, 3), np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        for kk, cands in CANDIDATES.items():
            sel = k == kk
            if not sel.any():
                continue
            Pk, Sk = P[sel], S[sel]
            best = ch = tb = None
            for ci, cand in enumerate(cands):
                tgt = np.stack([Sk[:, src] if src >= 0 else np.zeros_like(Sk[:, 0]) for src in cand], axis=1)
                e = np.zeros(Pk.shape[0], np.float64)
                for n in range(3):                                                     # tracks outer, axes inner, one running sum
                    for a in range(3):
                        d = Pk[:, n, a] - tgt[:, n, a]
                        e = e + d * d
                if ci == 0:
                    best, ch, tb = e, np.zeros(Pk.shape[0], np.uint8), tgt
                else:
                    better = e < best                                                  # strictly smaller only: NaN never displaces
                    best, ch, tb = np.where(better, e, best), np.where(better, np.uint8(ci), ch), np.where(better[:, None, None], tgt, tb)
            chosen[sel], e_min[sel], t_chosen[sel] = ch, best, tb
        item = e_min / 9.0
        denom = 9.0 * float(rows * C)
        g = ((2.0 * (P - t_chosen)) / denom).astype(np.float32)
    finite = np.isfinite(item).all()
    loss = math.fsum(item.ravel().tolist()) / float(rows * C) if finite else float('nan')
    return dict(chosen=chosen, item=item, g_doa=from_items(g), loss=loss, k=k)


def loss_bound(loss, rows, C, blocks=64, threads=256):
    """How far the kernel's float32 loss may lie from the exact one.  Every item is a non-negative float64, so each rounding of a
    partial sum is at most 2^-53 of the final sum; an item passes through at most ceil(items / (blocks threads)) additions in its
    thread, log2(threads) in the workgroup tree and `blocks` in the finish launch, then one division and one cast to float32
    (2^-24, or half the least subnormal).  First order, with 1 % on top for the second-order terms."""
    depth = -(-rows * C // (blocks * threads)) + int(math.log2(threads)) + blocks + 1
    return abs(loss) * (2.0 ** -24 + 1.01 * depth * 2.0 ** -53) + 2.0 ** -150


def torch_sum_bound(loss, rows, C):
    """the same for a float64 sum of the items in ANY order (at most items - 1 roundings per item), one division, one float32 cast"""
    return abs(loss) * (2.0 ** -24 + 1.01 * (rows * C + 1) * 2.0 ** -53) + 2.0 ** -150


def unit(rng, shape):
    v = rng.standard_normal(shape + (3,))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def build_adpit_inputs(rows, C, seed, ties=True, nan=False, prefix_only=False):
    """Random k = 0 .. 3 mixtures: predictions N(0, 0.7), slot targets unit vectors (zero where inactive).  ties: item 0 of a few rows
    gets two tracks with equal predictions and two slots with equal targets (exact cost ties); the activity patterns include
    non-prefix ones unless prefix_only.  nan: one prediction is NaN."""
    rng = np.random.default_rng(seed)
    P = (0.7 * rng.standard_normal((rows, C, 3, 3))).astype(np.float32)
    k = rng.integers(0, 4, (rows, C))
    s = np.arange(3)[None, None, :] < k[..., None]
    if not prefix_only:
        perm = np.argsort(rng.random((rows, C, 3)), axis=-1)
        shuffle = rng.random((rows, C)) < 0.25
        s = np.where(shuffle[..., None], np.take_along_axis(s, perm, axis=-1), s)
    T = (unit(rng, (rows, C, 3)) * s[..., None]).astype(np.float32)
    if ties:
        for r in range(0, rows, max(1, rows // 5)):
            c = r % C
            s[r, c] = True
            T[r, c] = unit(rng, (3,)).astype(np.float32)
            if r % 2 == 0:
                T[r, c, 1] = T[r, c, 0]                                                # two slots, one target
            P[r, c, 1] = P[r, c, 0]                                                    # two tracks, one prediction
    if nan:
        P[rows // 2, C // 2, 1, 2] = np.nan
    sed = np.ascontiguousarray(s.transpose(0, 2, 1)).reshape(rows, 3 * C).astype(np.float32)
    return from_items(P), sed, from_items(T)


# ------------------------------------------------------------------------------------------------------------------ decoder
def angles(x, y, z):
    """integer degrees of float32 components, in float64: round-half-even, azimuth 180 -> -180, a NaN angle -> 0"""
    x, y, z = float(x), float(y), float(z)
    a = np.arctan2(y, x) * 180.0 / np.pi
    e = np.arctan2(z, np.sqrt(x * x + y * y)) * 180.0 / np.pi
    azi = 0 if a != a else int(np.rint(a))
    ele = 0 if e != e else int(np.rint(e))
    return (-180 if azi == 180 else azi), ele


def similar(ai, aj, vi, vj, cos_unify):
    if not (ai and aj):
        return False
    xi, yi, zi, xj, yj, zj = (np.float64(t) for t in (*vi, *vj))
    with np.errstate(invalid='ignore', over='ignore'):
        dot = (xi * xj + yi * yj) + zi * zj
        ni, nj = (xi * xi + yi * yi) + zi * zi, (xj * xj + yj * yj) + zj * zj
        return bool(dot > np.float64(cos_unify) * np.sqrt(ni * nj))


def unify_cell(act, v, threshold, cos_unify):
    """act (3,) float32, v (3, 3) float32 (track, axis) -> (list of emitted float32 vectors in group order, flags)"""
    a = [bool(np.float32(act[n]) >= np.float32(threshold)) for n in range(3)]
    s01, s12, s20 = similar(a[0], a[1], v[0], v[1], cos_unify), similar(a[1], a[2], v[1], v[2], cos_unify), similar(a[2], a[0], v[2], v[0], cos_unify)
    flags = int(s01) | int(s12) << 1 | int(s20) << 2 | int(a[0]) << 4 | int(a[1]) << 5 | int(a[2]) << 6
    n_sim = int(s01) + int(s12) + int(s20)
    with np.errstate(invalid='ignore', over='ignore'):
        if n_sim == 0:
            return [v[n] for n in range(3) if a[n]], flags
        if n_sim >= 2:
            return [((v[0] + v[1]) + v[2]) / np.float32(3.0)], flags
        i, j = (0, 1) if s01 else (1, 2) if s12 else (0, 2)
        other = 3 - i - j
        groups = [(i, (v[i] + v[j]) / np.float32(2.0))] + ([(other, v[other])] if a[other] else [])
    return [g[1] for g in sorted(groups, key=lambda g: g[0])], flags


def decode_reference(act, xyz, n_frames, C, threshold, cos_unify):
    """one file, cell by cell: act (>= n_frames, 3 C), xyz (.., 9 C) float32 -> rows (n, 4) int16, n_out (n_frames, C), flags
    (n_frames, C), out (n_frames, C, 3, 3) float32 (zero behind n_out)"""
    act, xyz = np.asarray(act, np.float32), np.asarray(xyz, np.float32)
    V = to_items(xyz[:n_frames], C)
    A = act[:n_frames].reshape(n_frames, 3, C).transpose(0, 2, 1)
    rows = []
    n_out, flags, out = np.zeros((n_frames, C), np.int32), np.zeros((n_frames, C), np.int32), np.zeros((n_frames, C, 3, 3), np.float32)
    for f in range(n_frames):
        for c in range(C):
            vecs, flags[f, c] = unify_cell(A[f, c], V[f, c], threshold, cos_unify)
            n_out[f, c] = len(vecs)
            for g, vec in enumerate(vecs):
                out[f, c, g] = vec
                rows.append((f, c) + angles(*vec))
    return np.asarray(rows, np.int16).reshape(-1, 4), n_out, flags, out


def _near_rounding_edge(vec, margin):
    """vec (..., 3) float32: does an angle of it lie within `margin` degrees of a half-degree rounding edge?"""
    v = vec.astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        a = np.arctan2(v[..., 1], v[..., 0]) * 180.0 / np.pi
        e = np.arctan2(v[..., 2], np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1])) * 180.0 / np.pi
    bad = np.zeros(v.shape[:-1], bool)
    for t in (a, e):
        frac = t - np.floor(t)
        bad |= np.abs(frac - 0.5) <= margin
    return bad


def _cell_candidates(V):
    """every vector a cell (.., track, axis) can emit: the three tracks, the three pair means, the mean of all three"""
    two, three = np.float32(2.0), np.float32(3.0)
    return np.stack([V[..., 0, :], V[..., 1, :], V[..., 2, :], (V[..., 0, :] + V[..., 1, :]) / two, (V[..., 1, :] + V[..., 2, :]) / two,
                     (V[..., 0, :] + V[..., 2, :]) / two, ((V[..., 0, :] + V[..., 1, :]) + V[..., 2, :]) / three], axis=-2)


def build_decode_inputs(files, n_in, C, seed, threshold=0.5, unify_deg=15.0, fill=None, margin=1e-6):
    """act (files, n_in, 3 C), xyz (files, n_in, 9 C) float32.  Track vectors: a random direction of length U(0.2, 1.2); a third of
    the cells get track 1 within 0.3 .. 1.3 unify_deg of track 0, half of those also track 2 within 0.3 .. 1.3 unify_deg of track 1 -- in a
    random plane or continuing the arc from track 0 (pairs and triples of every kind, chains 0 ~ 1 ~ 2 with 0 and 2 apart included).  Activities: sqrt(U(0, 1)) with a tenth exactly AT the threshold, a few NaN.  fill 'all': every track
    active and far apart (3 rows per cell); 'none': nothing active.  No angle any cell can emit lies within `margin` degrees of a
    half-degree rounding edge: such cells are redrawn, and the result is asserted -- a condition on the inputs, not a tolerance."""
    rng = np.random.default_rng(seed)
    shape = (files, n_in, C)

    def draw(shape):
        V = unit(rng, shape + (3,)) * rng.uniform(0.2, 1.2, shape + (3, 1))
        if fill != 'all':
            near = rng.random(shape) < 1 / 3
            near2 = near & (rng.random(shape) < 1 / 2)
            chain = (rng.random(shape) < 1 / 2)[..., None]                             # track 2 in the plane of tracks 0 and 1, beyond 1
            ang1, ang2 = (np.deg2rad(rng.uniform(0.3 * unify_deg, 1.3 * unify_deg, shape))[..., None] for _ in range(2))
            u0 = V[..., 0, :] / np.linalg.norm(V[..., 0, :], axis=-1, keepdims=True)
            w0 = np.cross(u0, unit(rng, shape))
            w0 /= np.linalg.norm(w0, axis=-1, keepdims=True)
            u1 = np.cos(ang1) * u0 + np.sin(ang1) * w0
            w1 = np.cross(u1, unit(rng, shape))
            w1 /= np.linalg.norm(w1, axis=-1, keepdims=True)
            u2 = np.where(chain, np.cos(ang1 + ang2) * u0 + np.sin(ang1 + ang2) * w0, np.cos(ang2) * u1 + np.sin(ang2) * w1)
            V[..., 1, :] = np.where(near[..., None], u1 * rng.uniform(0.2, 1.2, shape + (1,)), V[..., 1, :])
            V[..., 2, :] = np.where(near2[..., None], u2 * rng.uniform(0.2, 1.2, shape + (1,)), V[..., 2, :])
        else:                                                                          # three directions at right angles
            q = np.linalg.qr(rng.standard_normal(shape + (3, 3)))[0]
            V = q * rng.uniform(0.6, 1.2, shape + (3, 1))
        return V.astype(np.float32)

    V = draw(shape)
    for _ in range(20):
        bad = _near_rounding_edge(_cell_candidates(V), margin).any(-1)
        if not bad.any():
            break
        V[bad] = draw((int(bad.sum()),))
    assert not _near_rounding_edge(_cell_candidates(V), margin).any(), 'an angle within the margin of a rounding edge'
    act = np.sqrt(rng.random(shape + (3,))).astype(np.float32)                          # (three in four above 0.5)
    act[rng.random(shape + (3,)) < 0.1] = np.float32(threshold)
    act[rng.random(shape + (3,)) < 0.01] = np.nan
    if fill == 'all':
        act[:] = np.float32(threshold) + rng.random(shape + (3,)).astype(np.float32)
    elif fill == 'none':
        act[:] = np.nextafter(np.float32(threshold), np.float32(-1)) * rng.random(shape + (3,)).astype(np.float32)
    act = np.ascontiguousarray(act.transpose(0, 1, 3, 2)).reshape(files, n_in, 3 * C)
    xyz = np.ascontiguousarray(V.transpose(0, 1, 4, 3, 2)).reshape(files, n_in, 9 * C)  # (f, t, axis, track, c)
    return act, xyz


def knife_edge_pair(seed):
    """two float32 vectors and their cosine c0 = dot / sqrt(ni nj) by the decoder's own float64 statements: cos_unify a few ulps below
    c0 makes the pair similar (dot > cos_unify sqrt(.)), at or above c0 not (up to the rounding of the product, which the product
    code and this file evaluate by the same statements)"""
    rng = np.random.default_rng(seed)
    vi = (unit(rng, ()) * 0.9).astype(np.float32)
    vj = (unit(rng, ()) * 0.7 + vi).astype(np.float32)
    xi, yi, zi, xj, yj, zj = (np.float64(t) for t in (*vi, *vj))
    dot = (xi * xj + yi * yj) + zi * zj
    c0 = dot / np.sqrt(((xi * xi + yi * yi) + zi * zi) * ((xj * xj + yj * yj) + zj * zj))
    return vi, vj, float(c0)


# ------------------------------------------------------------------------------------------------------------------ 13-way form
def adpit_13way(doa, sed_gt, doa_gt, C):
    """The DCASE 2022 baseline's formulation on this layout, in torch float64 (autograd): the label is split into the dummy-padded
    target sets A0 (one source), B0 B1 (two), C0 C1 C2 (three) -- a set is the slots' targets where the item has exactly that many
    active slots and zero elsewhere; 13 candidate target triples are formed; each candidate's padding adds the targets of the OTHER
    set sizes (which are zero or hold the item's own set), and the loss is the minimum over the 13 of the mean squared error over
    the 9 components, averaged over the items.  -> scalar float64 tensor."""
    import torch
    rows = doa.shape[0]
    P = doa.double().reshape(rows, 3, 3, C).permute(0, 3, 2, 1)                         # (rows, C, track, axis)
    T = doa_gt.double().reshape(rows, 3, 3, C).permute(0, 3, 2, 1)
    s = sed_gt.reshape(rows, 3, C).permute(0, 2, 1) > 0.5
    order = torch.argsort((~s).to(torch.int8), dim=-1, stable=True)
    S = torch.gather(T, 2, order[..., None].expand(-1, -1, -1, 3))
    k = s.sum(-1)[..., None]                                                            # (rows, C, 1)
    zero = torch.zeros_like(S[:, :, 0])
    A0 = torch.where(k == 1, S[:, :, 0], zero)
    B0, B1 = torch.where(k == 2, S[:, :, 0], zero), torch.where(k == 2, S[:, :, 1], zero)
    C0, C1, C2 = (torch.where(k == 3, S[:, :, i], zero) for i in range(3))
    st = lambda *t: torch.stack(t, dim=2)                                               # noqa: E731
    cands = [st(A0, A0, A0), st(B0, B0, B1), st(B0, B1, B0), st(B0, B1, B1), st(B1, B0, B0), st(B1, B0, B1), st(B1, B1, B0),
             st(C0, C1, C2), st(C0, C2, C1), st(C1, C0, C2), st(C1, C2, C0), st(C2, C0, C1), st(C2, C1, C0)]
    pad_a, pad_b, pad_c = cands[1] + cands[7], cands[0] + cands[7], cands[0] + cands[1]
    losses = []
    for i, t in enumerate(cands):
        t = t + (pad_a if i == 0 else pad_b if i < 7 else pad_c)
        losses.append(((P - t) ** 2).mean(dim=(2, 3)))
    return torch.stack(losses).min(dim=0).values.mean()
