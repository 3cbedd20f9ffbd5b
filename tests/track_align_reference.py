"""The restatement the track-alignment tests compare against, statement for statement in numpy; it imports
nothing from salsa_amd (but for the stub forward at the end, which takes its activities from nn_ops.accdoa_sed).  Layout: a row of 9 C columns holds component (axis a, track n, class c) at column (3 a + n) C + c, a row of
3 C columns the activity of (track n, class c) at n C + c.

  align        cost of candidate pi = sum over tracks (outer) and axes (inner) of (R[n][a] - V[pi(n)][a])^2, one running float64 sum;
               the six permutations in dictionary order; a later candidate wins only when strictly smaller
  merge        every slab un-swapped, every slab after the first aligned to slab 0 alone, float32 adds in slab order starting from
               slab 0, one division by float32(N); activities = sqrt((x x + y y) + z z) in float32
  combine      the per-frame walk of the chunk combine: the chunks over a frame in chunk order, the leftover chunk last; chunk 0 and
               a frame behind the overlap overwrite, otherwise align to the running value and (old + new[pi]) / 2"""
import itertools

import numpy as np

PERMS = tuple(itertools.permutations(range(3)))             # dictionary order: 012 021 102 120 201 210
KIND = {'foa': 1, 'mic': 2, 'gcc': 3}
V = {'foa': 16, 'mic': 8, 'gcc': 4}
F32 = np.float32


def bits(kind, v):
    assert 0 <= v < V[kind]
    if kind == 'gcc':
        return [int(v == 1), int(v == 2), int(v == 3), 0]
    return [(v >> j) & 1 for j in range(4)] if kind == 'foa' else [(v >> j) & 1 for j in range(3)] + [0]


def cells_of(xyz, C):
    """(..., 9 C) -> (..., C, track, axis)"""
    return np.moveaxis(xyz.reshape(xyz.shape[:-1] + (3, 3, C)), (-3, -2, -1), (-1, -2, -3))


def rows_of(cells):
    """(..., C, track, axis) -> (..., 9 C)"""
    C = cells.shape[-3]
    return np.ascontiguousarray(np.moveaxis(cells, (-1, -2, -3), (-3, -2, -1))).reshape(cells.shape[:-3] + (9 * C,))


def acts_of(act, C):
    """(..., 3 C) -> (..., C, track)"""
    return np.swapaxes(act.reshape(act.shape[:-1] + (3, C)), -1, -2)


def act_rows_of(a):
    C = a.shape[-2]
    return np.ascontiguousarray(np.swapaxes(a, -1, -2)).reshape(a.shape[:-2] + (3 * C,))


def unswap_cells(cells, kind, v):
    """S_m^-1 on (..., track, axis) cells: the steps of the swap in reverse bit order (selection and negation only)"""
    m = bits(kind, v)
    x, y, z = cells[..., 0].copy(), cells[..., 1].copy(), cells[..., 2].copy()
    if kind == 'foa':
        x, y, z = (-x if m[1] else x), (-y if m[2] else y), (-z if m[3] else z)
    else:
        if m[2]:
            y, z = -y, -z
        if m[1]:
            x, y = -y, -x
    if m[0]:
        x, y = y, x
    return np.stack([x, y, z], axis=-1)


def swap_cells(cells, kind, v):
    """S_m: the inverse of unswap_cells (bit 0 first)"""
    m = bits(kind, v)
    x, y, z = cells[..., 0].copy(), cells[..., 1].copy(), cells[..., 2].copy()
    if m[0]:
        x, y = y, x
    if kind == 'foa':
        x, y, z = (-x if m[1] else x), (-y if m[2] else y), (-z if m[3] else z)
    else:
        if m[1]:
            x, y = -y, -x
        if m[2]:
            y, z = -y, -z
    return np.stack([x, y, z], axis=-1)


def costs(R, Vc):
    """R, Vc (..., track, axis) float32 -> the six candidate costs (6, ...) float64"""
    R, Vc = R.astype(np.float64), Vc.astype(np.float64)
    out = []
    with np.errstate(invalid='ignore', over='ignore'):
        for perm in PERMS:
            e = np.zeros(R.shape[:-2])
            for n in range(3):
                for a in range(3):
                    d = R[..., n, a] - Vc[..., perm[n], a]
                    e = e + d * d
            out.append(e)
    return np.stack(out)


def align(R, Vc):
    e = costs(R, Vc)
    chosen, best = np.zeros(e.shape[1:], np.int32), e[0]
    for cand in range(1, 6):
        less = e[cand] < best                                   # (False for a NaN on either side)
        best, chosen = np.where(less, e[cand], best), np.where(less, np.int32(cand), chosen)
    return chosen


def permuted(x, cand):
    """x (..., track, ...) with one trailing axis or none after the track axis; cand (...) -> x[..., PERMS[cand][n], ...]"""
    src = np.asarray(PERMS)[cand]                              # (..., track)
    if x.ndim == src.ndim:
        return np.take_along_axis(x, src, axis=-1)
    return np.take_along_axis(x, src[..., None], axis=-2)


def merge(xyz_slab, n_models, ids, kind, C, align_tracks=True):
    """xyz_slab (N, B, L, 9 C) float32 -> act (B, L, 3 C), xyz (B, L, 9 C), perm (N, B, L, C) int32; align_tracks False: the plain
    section 9h merge, track n with track n"""
    N = xyz_slab.shape[0]
    assert N == n_models * len(ids)
    perm = np.zeros(xyz_slab.shape[:3] + (C,), np.int32)
    R = acc = None
    with np.errstate(invalid='ignore', over='ignore'):
        for k in range(N):
            Vc = unswap_cells(cells_of(xyz_slab[k], C), kind, ids[k % len(ids)])
            if k == 0:
                R = acc = Vc
                continue
            if align_tracks:
                perm[k] = align(R, Vc)
                Vc = permuted(Vc, perm[k])
            acc = acc + Vc
        out = (acc / F32(N)).astype(F32)
        x, y, z = out[..., 0], out[..., 1], out[..., 2]
        act = np.sqrt((x * x + y * y) + z * z)
    return act_rows_of(act), rows_of(out), perm


def starts_of(n_frames, chunk_len, hop):
    if chunk_len >= n_frames:
        return [0]
    s = list(range(0, n_frames - chunk_len + 1, hop))
    if (n_frames - chunk_len) % hop:
        s.append(n_frames - chunk_len)
    return s


def combine(act, xyz, chunk_len, hop, n_frames, C):
    """one file: act (n_chunks, chunk_len, 3 C), xyz (.., 9 C) -> (n_frames, 3 C), (n_frames, 9 C), and per frame the chunk whose
    track order the result carries (the last one that overwrote)"""
    starts = starts_of(n_frames, chunk_len, hop)
    assert len(starts) == act.shape[0]
    a, v = acts_of(act, C), cells_of(xyz, C)                  # (chunk, frame, C, track[, axis])
    out_a, out_v = np.zeros((n_frames, C, 3), F32), np.zeros((n_frames, C, 3, 3), F32)
    owner = np.zeros(n_frames, np.int64)
    overlap = chunk_len - hop
    with np.errstate(invalid='ignore', over='ignore'):
        for f in range(n_frames):
            for i, s in enumerate(starts):                     # (the leftover chunk is the last start)
                off = f - s
                if not 0 <= off < chunk_len:
                    continue
                if len(starts) == 1 or i == 0 or off >= overlap:
                    out_a[f], out_v[f], owner[f] = a[i, off], v[i, off], i
                    continue
                cand = align(out_v[f], v[i, off])
                out_v[f] = (out_v[f] + permuted(v[i, off], cand)) / F32(2.0)
                out_a[f] = (out_a[f] + permuted(a[i, off], cand)) / F32(2.0)
    return act_rows_of(out_a), rows_of(out_v), owner


# ------------------------------------------------------------------------------------------------------------------ built cells
def special_cells(seed):
    """(name, R (track, axis), V (track, axis), expected candidate or None) cells on which the walk's rules decide: exact ties, costs
    one ulp apart in either direction, NaN"""
    rng = np.random.default_rng(seed)
    u = lambda *s: rng.uniform(-1, 1, s).astype(F32)
    out = []
    R = u(3, 3)
    out.append(('two zero tracks', R, np.stack([u(3), np.zeros(3, F32), np.zeros(3, F32)]), None))
    out.append(('three zero tracks', R, np.zeros((3, 3), F32), 0))
    t = u(3)
    out.append(('duplicated tracks', R, np.stack([t, t, t]), 0))            # ADPIT's k = 1 target: all six tie
    out.append(('two duplicated tracks', R, np.stack([u(3), t, t]), None))
    Vn = u(3, 3)
    Vn[1, 2] = np.nan
    out.append(('NaN in the incoming cell', R, Vn, 0))
    Rn = u(3, 3)
    Rn[0, 0] = np.nan
    out.append(('NaN in the anchor', Rn, Vn[::-1].copy(), 0))
    # duplicated ANCHOR tracks 1 and 2: candidates 0 and 1 add the same nine squares in another order, so their float64 sums differ by
    # rounding alone; the search keeps one cell per direction where the two are exactly one ulp apart and no other candidate is lower
    want = {-1: None, 1: None}
    while any(w is None for w in want.values()):
        Rd, Vd = u(3, 3), u(3, 3)
        Rd[2] = Rd[1]
        e = costs(Rd, Vd)
        lo, hi = min(e[0], e[1]), max(e[0], e[1])
        if lo != hi and np.nextafter(lo, np.inf) == hi and lo < e[2:].min():
            want[-1 if e[1] < e[0] else 1] = (Rd, Vd)
    out.append(('candidate 1 one ulp below candidate 0', want[-1][0], want[-1][1], 1))
    out.append(('candidate 1 one ulp above candidate 0', want[1][0], want[1][1], 0))
    return out


def random_slab(N, B, L, C, seed):
    """(N, B, L, 9 C) float32 in [-1, 1] with signed zeros and values at +-1 mixed in"""
    rng = np.random.default_rng(seed)
    x = np.tanh(2 * rng.standard_normal((N, B, L, 9 * C))).astype(F32)
    special = np.array([0.0, -0.0, 1.0, -1.0, 2.0 ** -149], F32)
    pick = rng.random(x.shape) < 0.1
    x[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    return x


def near_slab(N, B, L, C, seed):
    """random_slab whose later slabs are slab 0 moved a little, with every cell's tracks shuffled: close calls and a mix of candidates"""
    x = random_slab(N, B, L, C, seed)
    for k in range(1, N):
        cells, _ = shuffled(cells_of((x[k] * F32(0.05) + x[0]).astype(F32), C), seed + k)
        x[k] = rows_of(cells)
    return x


def plant_special(xyz_slab, ids, kind, C, seed):
    """write special_cells into the first cells of the slab (un-swapped domain: slab k holds S_m of the cell): anchor in slab 0, the
    incoming cell in every later slab.  Returns the number of cells written."""
    N = xyz_slab.shape[0]
    cells = special_cells(seed)
    flat = [cells_of(xyz_slab[k], C).copy().reshape(-1, 3, 3) for k in range(N)]
    n = min(len(cells), flat[0].shape[0])
    for j in range(n):
        _, R, Vc, _ = cells[j]
        for k in range(N):
            flat[k][j] = swap_cells(R if k == 0 else Vc, kind, ids[k % len(ids)])
    for k in range(N):
        xyz_slab[k] = rows_of(flat[k].reshape(xyz_slab.shape[1:3] + (C, 3, 3)))
    return n


def planted_tracks(shape, seed):
    """base tracks (shape..., track, axis) float32 with pairwise distance >= 0.5 between the three tracks of a cell: three corners of a
    cube of side 0.6 (distance >= 0.6) moved by less than 0.02 per component (2 sqrt(3) 0.02 < 0.07)"""
    rng = np.random.default_rng(seed)
    corners = np.array(list(itertools.product((-0.3, 0.3), repeat=3)))
    pick = np.argsort(rng.random(shape + (8,)), axis=-1)[..., :3]
    base = corners[pick] + rng.uniform(-0.02, 0.02, shape + (3, 3))
    base = base.astype(F32)
    d = np.linalg.norm(base[..., [0, 1, 2], :].astype(np.float64) - base[..., [1, 2, 0], :].astype(np.float64), axis=-1)
    assert d.min() >= 0.5
    return base


def shuffled(cells, seed):
    """cells (..., track, axis), a seeded permutation per cell -> (cells with track n = the original track sigma[n], sigma (..., track))"""
    rng = np.random.default_rng(seed)
    sigma = np.asarray(PERMS)[rng.integers(0, 6, cells.shape[:-2])]
    return np.take_along_axis(cells, sigma[..., None], axis=-2), sigma


def cand_of(perm_rows):
    """(..., track) permutations -> their candidate indices"""
    table = {p: i for i, p in enumerate(PERMS)}
    flat = perm_rows.reshape(-1, 3)
    return np.array([table[tuple(int(t) for t in r)] for r in flat], np.int32).reshape(perm_rows.shape[:-1])


# ---------------------------------------------------------------------------------------------------------------- stub forward
def stub_forward(C_, shuffle_seed=None, pool=8):
    """An exactly FOA-equivariant Multi-ACCDOA forward of indexing, +, * and / only (bit-equal on any slice of the input): the
    component (axis a, track n, class c) is amp_n g(gain_n x[intensity row of a, frame, bin c]) with the odd g(r) = r / (1 + |r|), so a
    swapped input gives the swapped output bit for bit and a chunk gives the clip's frames.  shuffle_seed: the tracks of every cell
    are shuffled by a permutation drawn anew at every call (every chunk batch, every variant)."""
    import torch
    from salsa_amd.crnn.nn_ops import accdoa_sed
    calls = [0]

    def forward(x):
        b = x.shape[0]
        r = x[:, :, ::pool, :C_]                                                    # (b, 7, L, C)
        rows = (6, 4, 5)                                                            # Ix, Iy, Iz
        amp, gain = (1.0, 0.7, 0.4), (1.0, 3.0, 0.3)
        V = torch.stack([torch.stack([amp[n] * ((gain[n] * r[:, rows[a]]) / (1 + (gain[n] * r[:, rows[a]]).abs())) for n in range(3)], dim=2)
                         for a in range(3)], dim=2)                                 # (b, L, axis, track, C)
        if shuffle_seed is not None:
            g = torch.Generator().manual_seed(shuffle_seed + calls[0])
            sigma = torch.tensor(PERMS)[torch.randint(0, 6, (b, V.shape[1], C_), generator=g)].to(x.device)    # (b, L, C, track)
            V = torch.gather(V, 3, sigma.permute(0, 1, 3, 2)[:, :, None].expand_as(V))
        calls[0] += 1
        xyz = V.reshape(b, V.shape[1], 9 * C_).contiguous()
        return accdoa_sed(xyz, 3 * C_), xyz
    forward.calls = calls
    return forward
