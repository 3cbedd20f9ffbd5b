"""CPU tests of track_merge='align' (DESIGN.md section 9u): the per-cell arithmetic of salsa_nn_tta_merge_multi /
salsa_nn_chunk_merge_multi (salsa_amd/csrc/track_align.h built with g++: tests/hostemu/track_align_emu.cpp) and the product's numpy
and torch paths against the restatement of tests/track_align_reference.py, bit for bit; planted permutations; the keyword on
infer_pipelined, validate and TtaForward with stub forwards; and the launchers' argument checks on the built library."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import track_align_reference as ref
from conftest import ROOT

KINDS = ('foa', 'mic', 'gcc')
F32 = np.float32


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('track_align_emu') / 'libtrack_align_emu.so')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-o', so,
                           os.path.join(ROOT, 'tests', 'hostemu', 'track_align_emu.cpp')])
    L = C.CDLL(so)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    L.emu_align_cells.argtypes = [fp, fp, C.c_int64, ip]
    L.emu_merge.argtypes = [fp, C.c_int, ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, fp, fp, ip]
    L.emu_chunk_merge.argtypes = [fp, fp] + [C.c_int] * 6 + [fp, fp]
    return L


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def emu_align(emu, R, V):
    R, V = np.ascontiguousarray(R, F32).reshape(-1, 3, 3), np.ascontiguousarray(V, F32).reshape(-1, 3, 3)
    out = np.full(R.shape[0], -1, np.int32)
    emu.emu_align_cells(_fp(R), _fp(V), R.shape[0], _ip(out))
    return out


def emu_merge(emu, slab, n_models, ids, kind, C_):
    N, B, L, _ = slab.shape
    slab = np.ascontiguousarray(slab)
    xo, ao = np.full((B, L, 9 * C_), np.nan, F32), np.full((B, L, 3 * C_), np.nan, F32)
    perm = np.full((N, B, L, C_), -1, np.int32)
    assert emu.emu_merge(_fp(slab), n_models, (C.c_int * len(ids))(*ids), len(ids), ref.KIND[kind], B, L, C_, _fp(xo), _fp(ao), _ip(perm)) == 0
    return ao, xo, perm


def emu_chunks(emu, act, xyz, chunk_len, hop, n_frames, C_):
    files, n_chunks = act.shape[:2]
    act, xyz = np.ascontiguousarray(act), np.ascontiguousarray(xyz)
    fa, fx = np.full((files, n_frames, 3 * C_), np.nan, F32), np.full((files, n_frames, 9 * C_), np.nan, F32)
    assert emu.emu_chunk_merge(_fp(act), _fp(xyz), files, n_chunks, chunk_len, hop, n_frames, C_, _fp(fa), _fp(fx)) == 0
    return fa, fx


def chunk_case(files, n_frames, chunk_len, hop, C_, seed, special=True):
    n = len(ref.starts_of(n_frames, chunk_len, hop))
    xyz = ref.random_slab(files, n, chunk_len, C_, seed).copy()
    if special and n > 1 and chunk_len > hop:                 # the built cells meet in the first overlap: chunk 0's tail, chunk 1's head
        cells = ref.special_cells(seed)
        c0, c1 = ref.cells_of(xyz[0, 0], C_).copy(), ref.cells_of(xyz[0, 1], C_).copy()
        for j, (_, R, V, _) in enumerate(cells[:C_ * (chunk_len - hop)]):
            f, c = divmod(j, C_)
            c0[hop + f, c], c1[f, c] = R, V
        xyz[0, 0], xyz[0, 1] = ref.rows_of(c0), ref.rows_of(c1)
    cells = ref.cells_of(xyz, C_)
    with np.errstate(invalid='ignore'):
        act = ref.act_rows_of(np.sqrt((cells[..., 0] ** 2 + cells[..., 1] ** 2) + cells[..., 2] ** 2).astype(F32))
    return act, xyz


# ------------------------------------------------------------------------------------------------- 1. the definition, bit for bit
def test_candidate_table_is_the_adpit_table_in_dictionary_order():
    from salsa_amd.crnn.postprocess import TRACK_PERMS
    assert TRACK_PERMS == ref.PERMS == ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))


def test_align_cell_equals_the_restatement_on_random_and_built_cells(emu):
    from salsa_amd.crnn.postprocess import align_cells
    rng = np.random.default_rng(1)
    R, V = rng.uniform(-1, 1, (4000, 3, 3)).astype(F32), rng.uniform(-1, 1, (4000, 3, 3)).astype(F32)
    V[:2000] = np.take_along_axis(R[:2000], np.asarray(ref.PERMS)[rng.integers(0, 6, 2000)][..., None], axis=1) + \
        rng.uniform(-0.05, 0.05, (2000, 3, 3)).astype(F32)       # near-permutations of the anchor: every candidate gets chosen
    want = ref.align(R, V)
    assert set(want.tolist()) == set(range(6))
    assert np.array_equal(emu_align(emu, R, V), want) and np.array_equal(align_cells(R, V), want)
    cells = ref.special_cells(3)
    assert len(cells) == 8
    for name, Rc, Vc, expect in cells:
        got = int(emu_align(emu, Rc, Vc)[0])
        assert got == int(ref.align(Rc, Vc)) == int(align_cells(Rc, Vc)), name
        assert expect is None or got == expect, name
    e = ref.costs(cells[0][1], cells[0][2])                     # two zero tracks: candidates 0 and 1 tie exactly, the lower one stays
    assert e[0] == e[1] and int(emu_align(emu, cells[0][1], cells[0][2])[0]) in (0, 2, 4)
    for j, sign in ((6, -1), (7, 1)):                           # one ulp apart, in either direction
        e = ref.costs(cells[j][1], cells[j][2])
        assert np.nextafter(min(e[0], e[1]), np.inf) == max(e[0], e[1]) and (e[1] < e[0]) == (sign < 0)
    assert np.isnan(ref.costs(cells[4][1], cells[4][2])).all()


@pytest.mark.parametrize('kind,n_models,ids', [('foa', 1, [0]), ('foa', 1, [5, 0, 9]), ('gcc', 1, [0, 1, 2, 3]), ('mic', 2, [7, 3, 3, 1]),
                                               ('foa', 2, list(range(16)))])
@pytest.mark.parametrize('C_', [1, 13])
def test_merge_walk_equals_the_restatement(emu, kind, n_models, ids, C_):
    from salsa_amd.crnn.tta import tta_merge_multi
    N = n_models * len(ids)
    slab = ref.near_slab(N, 2, 5, C_, seed=N + C_)
    n_special = ref.plant_special(slab, ids, kind, C_, seed=7)
    want_a, want_x, want_p = ref.merge(slab, n_models, ids, kind, C_)
    got_a, got_x, got_p = emu_merge(emu, slab, n_models, ids, kind, C_)
    assert same_bits(got_x, want_x) and same_bits(got_a, want_a) and np.array_equal(got_p, want_p)
    assert N == 1 or n_special >= min(8, 10 * C_)
    a, x, p = tta_merge_multi(torch.from_numpy(slab), n_models, ids, kind, C_, return_perm=True)     # the CPU path of the product
    assert same_bits(x.numpy(), want_x) and same_bits(a.numpy(), want_a) and np.array_equal(p.numpy(), want_p)
    assert p.dtype == torch.int32 and len(tta_merge_multi(torch.from_numpy(slab), n_models, ids, kind, C_)) == 2


@pytest.mark.parametrize('kind', KINDS)
def test_torch_path_equals_numpy_for_every_variant_unswap_included(kind):
    from salsa_amd.crnn.tta import tta_merge_multi
    ids = list(range(ref.V[kind]))
    base = ref.planted_tracks((2, 4, 3), seed=5)               # well-separated tracks: a wrong un-swap cannot hide in the alignment
    slab = np.stack([ref.rows_of(ref.swap_cells(base, kind, v)) for v in ids])
    want_a, want_x, want_p = ref.merge(slab, 1, ids, kind, 3)
    # every slab rotates back onto slab 0 exactly: identical summands, so only the N - 1 additions and the division round
    assert not want_p.any() and np.abs(want_x - ref.rows_of(base)).max() <= len(ids) * 2.0 ** -24 * np.abs(base).max()
    for v in ids:                                               # the restatement's swap is the training augmentation's
        from salsa_amd.augment import swap_targets
        m = torch.tensor(ref.bits(kind, v)[:4 if kind == 'foa' else 3]).expand(2, -1)
        assert same_bits(swap_targets(torch.from_numpy(ref.rows_of(base)), m, 'foa' if kind == 'foa' else 'mic', 9).numpy(), slab[v]), v
    a, x, p = tta_merge_multi(torch.from_numpy(slab), 1, ids, kind, 3, return_perm=True)
    assert same_bits(x.numpy(), want_x) and same_bits(a.numpy(), want_a) and np.array_equal(p.numpy(), want_p)


CHUNK_CASES = [(23, 8, 3), (24, 8, 4), (20, 5, 5), (5, 8, 8), (24, 8, 3)]      # the last one ends in a leftover chunk


@pytest.mark.parametrize('n_frames,chunk_len,hop', CHUNK_CASES)
@pytest.mark.parametrize('C_', [1, 13])
def test_chunk_walk_equals_the_restatement(emu, n_frames, chunk_len, hop, C_):
    from salsa_amd.crnn.postprocess import combine_chunks_multi
    act, xyz = chunk_case(2, n_frames, chunk_len, hop, C_, seed=n_frames + C_)
    fa, fx = emu_chunks(emu, act, xyz, chunk_len, hop, n_frames, C_)
    for f in range(2):
        want_a, want_x, _ = ref.combine(act[f], xyz[f], chunk_len, hop, n_frames, C_)
        assert same_bits(fa[f], want_a) and same_bits(fx[f], want_x)
        host_a, host_x = combine_chunks_multi(act[f], xyz[f], chunk_len, hop, n_frames, C_)        # what decode='host' runs
        assert same_bits(host_a, want_a) and same_bits(host_x, want_x)


@pytest.mark.parametrize('n_frames,chunk_len,hop', [(20, 5, 5), (5, 8, 8), (7, 7, 3)])
def test_hop_equal_to_length_and_one_chunk_are_the_reshape(emu, n_frames, chunk_len, hop):
    from salsa_amd.crnn.postprocess import combine_chunks_multi
    act, xyz = chunk_case(2, n_frames, chunk_len, hop, 4, seed=2)
    fa, fx = emu_chunks(emu, act, xyz, chunk_len, hop, n_frames, 4)
    assert same_bits(fa, act.reshape(2, -1, 12)[:, :n_frames]) and same_bits(fx, xyz.reshape(2, -1, 36)[:, :n_frames])
    host = combine_chunks_multi(act[1], xyz[1], chunk_len, hop, n_frames, 4)
    assert same_bits(host[0], fa[1]) and same_bits(host[1], fx[1])


# ------------------------------------------------------------------------------------------------------ 2. planted permutations
def planted_slabs(N, B, L, C_, kind, ids, seed):
    """base tracks at pairwise distance >= 0.5, every slab the base moved by at most 0.01 per component; -> (the slabs with each cell's
    tracks shuffled by a seeded permutation, the unshuffled slabs, the permutations (N, B, L, C, track)), all swapped by the variant"""
    base = ref.planted_tracks((B, L, C_), seed)
    rng = np.random.default_rng(seed + 1)
    plain, mixed, sigmas = [], [], []
    for k in range(N):
        cells = (base + rng.uniform(-0.01, 0.01, base.shape)).astype(F32)
        sh, sigma = ref.shuffled(cells, seed + 2 + k)
        plain.append(ref.rows_of(ref.swap_cells(cells, kind, ids[k % len(ids)])))
        mixed.append(ref.rows_of(ref.swap_cells(sh, kind, ids[k % len(ids)])))
        sigmas.append(sigma)
    return np.stack(mixed), np.stack(plain), np.stack(sigmas)


@pytest.mark.parametrize('kind,n_models,ids', [('foa', 2, list(range(16))), ('mic', 1, [3, 0, 6]), ('gcc', 2, [1, 3])])
def test_planted_permutations_are_undone_by_the_merge(emu, kind, n_models, ids):
    """The right assignment costs at most 9 (2 x 0.01)^2 = 36 x 0.01^2 = 0.0036, any wrong one moves two tracks by at least
    0.5 - 2 sqrt(3) 0.01 each: at least 2 (0.5 - 0.035)^2 > 0.43.  The choice is forced, so the merge equals the plain section 9h merge
    of the unshuffled slabs, bit for bit, in slab 0's own track order, and the candidates are the planted ones."""
    from salsa_amd.crnn.tta import tta_merge_multi
    N, C_ = n_models * len(ids), 5
    mixed, plain, sigma = planted_slabs(N, 3, 7, C_, kind, ids, seed=11)
    _, plain_x, _ = ref.merge(plain, n_models, ids, kind, C_, align_tracks=False)
    want_cells = np.take_along_axis(ref.cells_of(plain_x, C_), sigma[0][..., None], axis=-2)
    inv = np.argsort(sigma, axis=-1)                            # sigma_k^-1
    want_p = ref.cand_of(np.take_along_axis(inv, np.broadcast_to(sigma[0], sigma.shape), axis=-1))   # pi = sigma_k^-1 o sigma_0
    assert not want_p[0].any() and len(set(want_p[1:].ravel().tolist())) == 6
    for got in (emu_merge(emu, mixed, n_models, ids, kind, C_),
                tuple(t.numpy() for t in tta_merge_multi(torch.from_numpy(mixed), n_models, ids, kind, C_, return_perm=True))):
        assert same_bits(got[1], ref.rows_of(want_cells)) and np.array_equal(got[2], want_p)
    # slab 0 unshuffled: the candidates are the planted inverses themselves
    mixed[0], sigma[0] = plain[0], np.arange(3)
    _, _, p = tta_merge_multi(torch.from_numpy(mixed), n_models, ids, kind, C_, return_perm=True)
    assert np.array_equal(p.numpy()[1:], ref.cand_of(inv[1:]))


@pytest.mark.parametrize('n_frames,chunk_len,hop', [(23, 8, 3), (24, 8, 4), (24, 8, 3)])
def test_planted_permutations_are_undone_by_the_chunk_combine(emu, n_frames, chunk_len, hop):
    """the same construction against combine_chunks applied column-wise to the unshuffled chunks: the result carries, frame by frame,
    the track order of the last chunk that overwrote the frame"""
    from salsa_amd.crnn.postprocess import combine_chunks, combine_chunks_multi
    C_, starts = 4, ref.starts_of(n_frames, chunk_len, hop)
    base = ref.planted_tracks((n_frames, C_), seed=n_frames)
    rng = np.random.default_rng(3)
    plain_x, plain_a, mixed_x, mixed_a, sigmas = [], [], [], [], []
    for i, s in enumerate(starts):
        cells = (base[s:s + chunk_len] + rng.uniform(-0.01, 0.01, (chunk_len, C_, 3, 3))).astype(F32)
        acts = rng.uniform(0, 1, (chunk_len, C_, 3)).astype(F32)
        sh, sigma = ref.shuffled(cells, 100 + i)
        plain_x.append(ref.rows_of(cells)), plain_a.append(ref.act_rows_of(acts))
        mixed_x.append(ref.rows_of(sh)), mixed_a.append(ref.act_rows_of(np.take_along_axis(acts, sigma, axis=-1)))
        sigmas.append(sigma)
    want_x = combine_chunks(np.stack(plain_x), chunk_len, hop, n_frames)
    want_a = combine_chunks(np.stack(plain_a), chunk_len, hop, n_frames)
    _, _, owner = ref.combine(np.stack(mixed_a), np.stack(mixed_x), chunk_len, hop, n_frames, C_)
    assert len(set(owner.tolist())) > 1
    own_sigma = np.stack([sigmas[owner[f]][f - starts[owner[f]]] for f in range(n_frames)])         # (frame, C, track)
    want_x = ref.rows_of(np.take_along_axis(ref.cells_of(want_x, C_), own_sigma[..., None], axis=-2))
    want_a = ref.act_rows_of(np.take_along_axis(ref.acts_of(want_a, C_), own_sigma, axis=-1))
    fa, fx = emu_chunks(emu, np.stack(mixed_a)[None], np.stack(mixed_x)[None], chunk_len, hop, n_frames, C_)
    assert same_bits(fx[0], want_x) and same_bits(fa[0], want_a)
    host_a, host_x = combine_chunks_multi(np.stack(mixed_a), np.stack(mixed_x), chunk_len, hop, n_frames, C_)
    assert same_bits(host_x, want_x) and same_bits(host_a, want_a)


# ------------------------------------------------------------------------------------------------------------ 3. the keyword
stub_forward = ref.stub_forward


def sorted_rows(rows):
    return [sorted(map(tuple, r)) for r in rows]


@pytest.mark.parametrize('mode', ['chunks', 'tta', 'both'])
def test_infer_pipelined_aligned_rows_are_those_of_the_unshuffled_stub(mode):
    from salsa_amd.crnn.infer import infer_clips_sharded, infer_pipelined
    feats = torch.randn(3, 7, 160, 8, generator=torch.Generator().manual_seed(4)) * 2
    kw = dict(sub_batch=2, sed_threshold=0.35, n_label_frames=20, decode='host', output_format='multi_accdoa', n_classes=4,
              eval_version='2020', unify_deg=0.001)
    extra = dict(track_merge='align')
    if mode == 'chunks':
        extra.update(chunk_len=64, chunk_hop_len=24, chunk_batch=3)                 # label chunks of 8 at hop 3: triple overlap
    if mode == 'both':
        extra.update(chunk_len=64, chunk_hop_len=40)                                # ... of 8 at hop 5: three chunks and a leftover one
    if mode in ('tta', 'both'):
        extra.update(tta=('foa', 'salsa'))
    # chunks of the stub repeat the clip's frames bit for bit and (v + v) / 2 is exact: the whole-clip rows.  Sixteen equal summands
    # do round (3 v is not a float32), so with tta= the yardstick is the unshuffled stub through the same merges, where every
    # alignment is the identity at cost 0: the shuffled run adds the same values in the same order, cell by cell.
    want = infer_pipelined(3, lambda lo, hi: feats[lo:hi], stub_forward(4), **(kw if mode == 'chunks' else dict(kw, **extra)))
    assert 100 < sum(len(r) for r in want) < 3 * 20 * 4 * 3
    fwd = stub_forward(4, shuffle_seed=9)
    rows = infer_pipelined(3, lambda lo, hi: feats[lo:hi], fwd, **dict(kw, **extra))
    assert fwd.calls[0] > 2 and sorted_rows(rows) == sorted_rows(want)
    out = infer_clips_sharded(['b', 'a', 'c'], lambda ns: feats[['abc'.index(n) for n in ns]], stub_forward(4, shuffle_seed=9), **dict(kw, **extra))
    assert sorted_rows([out[n] for n in 'abc']) == sorted_rows(want)
    # a merge of track n with track n would not do: the shuffled forwards, averaged as they come, give other rows
    if mode == 'chunks':
        from salsa_amd.crnn.postprocess import combine_chunks, multi_accdoa_rows
        from salsa_amd.crnn.decode import split_test_chunks
        p, d = stub_forward(4, shuffle_seed=9)(split_test_chunks(feats[:1], 64, 24))
        naive = multi_accdoa_rows(combine_chunks(p.numpy(), 8, 3, 20), combine_chunks(d.numpy(), 8, 3, 20), sed_threshold=0.35,
                                  unify_deg=0.001, n_classes=4, max_nframes_per_file=20, eval_version='2020')
        assert sorted(map(tuple, naive)) != sorted_rows(want)[0]


def test_refusals_of_the_keyword():
    from salsa_amd.crnn.infer import infer_pipelined
    from salsa_amd.crnn.tta import TtaForward, wrap_forward
    from salsa_amd.crnn.train import Trainer
    feats = torch.zeros(2, 7, 80, 8)
    kw = dict(sub_batch=2, n_label_frames=10, decode='host', output_format='multi_accdoa', n_classes=4)
    fwd = stub_forward(4)
    run = lambda **k: infer_pipelined(2, lambda lo, hi: feats[lo:hi], fwd, **dict(kw, **k))
    with pytest.raises(ValueError, match='overlap'):                                 # without the keyword both still raise
        run(chunk_len=40, chunk_hop_len=20)
    with pytest.raises(ValueError, match='test-time augmentation'):
        run(tta=('foa', 'salsa'))
    with pytest.raises(ValueError, match='gmean'):
        run(chunk_len=40, chunk_hop_len=20, track_merge='align', combine_method='gmean')
    run(chunk_len=40, chunk_hop_len=40, track_merge='align', combine_method='gmean')  # (no overlap: nothing is averaged)
    for fmt in ('reg_xyz', 'accdoa'):
        with pytest.raises(ValueError, match='track_merge'):
            run(track_merge='align', output_format=fmt)
        with pytest.raises(ValueError, match='track_merge'):
            TtaForward(fwd, 'foa', 'salsa', output_format=fmt, track_merge='align')
    for bad in ('mean', 'Align', True, 0):
        with pytest.raises(ValueError, match='track_merge'):
            run(track_merge=bad)
        with pytest.raises(ValueError, match='track_merge'):
            TtaForward(fwd, 'foa', 'salsa', output_format='multi_accdoa', track_merge=bad)
    assert fwd.calls[0] == 1                                                         # (only the accepted run reached the forward)
    with pytest.raises(ValueError, match='test-time augmentation'):
        TtaForward(fwd, 'foa', 'salsa', output_format='multi_accdoa')
    with pytest.raises(ValueError, match='built without'):
        wrap_forward(fwd, TtaForward(fwd, 'foa', 'salsa'), 4, 'multi_accdoa', 'align')
    tf = TtaForward(fwd, 'foa', 'salsa', n_classes=4, output_format='multi_accdoa', track_merge='align')
    assert wrap_forward(None, tf, 4, 'multi_accdoa', 'align') is tf and tf._prob is None
    with pytest.raises(ValueError, match='expected'):
        TtaForward(stub_forward(5), 'foa', 'salsa', n_classes=4, output_format='multi_accdoa', track_merge='align')(feats)
    tr = Trainer('cpu', amp_dtype=None, output_format='multi_accdoa', n_classes=2, decoder_size=32)
    x = torch.randn(1, 7, 32, 200, generator=torch.Generator().manual_seed(1))
    with pytest.raises(ValueError, match='test-time augmentation'):
        tr.infer_tta(x, variants=[0, 5])
    tr.track_merge = 'align'
    act, xyz = tr.infer_tta(x, variants=[0, 5])
    assert act.shape == (1, 4, 6) and xyz.shape == (1, 4, 18)
    from salsa_amd.crnn.nn_ops import accdoa_sed
    assert torch.equal(act, accdoa_sed(xyz, 6))


def test_ttaforward_keeps_only_an_xyz_slab_and_returns_the_merged_lengths():
    from salsa_amd.crnn.nn_ops import accdoa_sed
    from salsa_amd.crnn.tta import TtaForward, tta_merge_multi, tta_variant
    x = torch.randn(2, 7, 32, 8, generator=torch.Generator().manual_seed(6))
    f1, f2 = stub_forward(3, shuffle_seed=1), stub_forward(3, shuffle_seed=50)
    tf = TtaForward([f1, f2], 'foa', 'salsa', variants=[4, 0, 11], n_classes=3, output_format='multi_accdoa', track_merge='align')
    act, xyz = tf(x)
    assert tf._prob is None and tf._xyz is not None and act.dtype == xyz.dtype == torch.float32
    assert act.shape == (2, 4, 9) and xyz.shape == (2, 4, 27) and torch.equal(act, accdoa_sed(xyz, 9))
    g1, g2 = stub_forward(3, shuffle_seed=1), stub_forward(3, shuffle_seed=50)       # the same calls by hand, slabs model-major
    outs = [[g(tta_variant(x, 'foa', v))[1] for g in (g1, g2)] for v in (4, 0, 11)]
    slab = torch.stack([outs[vi][mi] for mi in range(2) for vi in range(3)])
    want = tta_merge_multi(slab, 2, [4, 0, 11], 'foa', 3)
    assert torch.equal(xyz, want[1]) and torch.equal(act, want[0])


def test_validate_runs_with_chunks_and_tta_together_on_a_trackwise_bank():
    import inspect

    from salsa_amd.crnn import fit
    from salsa_amd.crnn.infer import infer_clips_sharded, infer_pipelined
    from salsa_amd.crnn.tta import TtaForward
    from salsa_amd.crnn.train import Trainer
    from salsa_amd.dataset import GpuFeatureBank
    for fn in (fit.validate, fit.fit, infer_pipelined, infer_clips_sharded):
        assert inspect.signature(fn).parameters['track_merge'].default is None
    tr = Trainer('cpu', amp_dtype=None, output_format='multi_accdoa', n_classes=2, decoder_size=32)
    bank = GpuFeatureBank(None, chunk_len_s=64 / 80, chunk_hop_len_s=64 / 80, n_classes=6, device='cpu', label_format='trackwise')
    bank.add_features(torch.randn(2, 7, 64, 200, generator=torch.Generator().manual_seed(2)), ['a', 'b'])
    bank.finalize(normalize=False)
    gt = [[(0, 1, 10, 0), (0, 1, 120, 5)], [(3, 0, -50, 0)]]
    tf = TtaForward(tr.infer, 'foa', 'salsa', variants=[0, 6], n_classes=2, output_format='multi_accdoa', track_merge='align')
    val = fit.validate(tr, bank, gt, chunk_len=32, chunk_hop_len=16, sed_threshold=0.0, sub_batch=2, return_rows=True, tta=tf,
                       track_merge='align')
    assert all(0 <= r[1] < 2 and 0 <= r[0] < 8 for rows in val['rows'] for r in rows) and len(val['rows'][0]) >= 8
    assert np.isfinite(val['valSeld'])
    with pytest.raises(ValueError, match='overlap'):
        fit.validate(tr, bank, gt, chunk_len=32, chunk_hop_len=16)
    with pytest.raises(ValueError, match='track_merge'):
        fit.validate(Trainer('cpu', amp_dtype=None, output_format='accdoa', n_classes=6, decoder_size=32), bank, gt, track_merge='align')
    with pytest.raises(ValueError, match='track_merge'):
        fit.fit(tr, bank, val_bank=bank, val_gt=gt, track_merge='best')


# ------------------------------------------------------------------------------------------------------------ 4. refusals
@pytest.fixture(scope='module')
def lib():
    from salsa_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_launchers_refuse_invalid_arguments_before_any_device_call(lib):
    """every call here returns -1 from the host-side checks with a message: nothing is launched, no pointer is read"""
    from salsa_amd import _lib
    assert 'salsa_nn_tta_merge_multi' in _lib.NN_EXPORTS and 'salsa_nn_chunk_merge_multi' in _lib.NN_EXPORTS
    assert os.path.join(ROOT, 'salsa_amd', 'csrc', 'track_align.hip') in _lib.build_command()
    vp, i = C.c_void_p, C.c_int
    assert _lib.PROTOTYPES['salsa_nn.h']['salsa_nn_tta_merge_multi'] == (i, [vp, i, vp, i, i, i, i, i, vp, vp, vp, vp])
    assert _lib.PROTOTYPES['salsa_nn.h']['salsa_nn_chunk_merge_multi'] == (i, [vp, vp, i, i, i, i, i, i, vp, vp, vp])
    p = [C.c_void_p(0x10000 * (k + 1)) for k in range(4)]
    ids = (C.c_int * 3)(5, 0, 9)
    good = dict(x=p[0], n_models=2, ids=ids, n=3, kind=1, B=3, L=7, C=13, xo=p[1], ao=p[2], perm=None)

    def merge(**kw):
        k = dict(good, **kw)
        return lib.salsa_nn_tta_merge_multi(k['x'], k['n_models'], k['ids'], k['n'], k['kind'], k['B'], k['L'], k['C'], k['xo'], k['ao'],
                                            k['perm'], None)
    for bad in (dict(kind=0), dict(kind=4), dict(ids=(C.c_int * 3)(5, 16, 9)), dict(ids=(C.c_int * 3)(5, -1, 9)), dict(kind=2), dict(kind=3),
                dict(n_models=0), dict(n=0), dict(n_models=-1), dict(n_models=4097), dict(n=17, ids=(C.c_int * 17)()), dict(x=None),
                dict(ids=None), dict(xo=None), dict(ao=None), dict(B=0), dict(L=0), dict(C=0), dict(B=1 << 16, L=1 << 15, C=1),
                dict(B=1 << 10, L=1 << 10, C=40), dict(B=1 << 14, L=600, C=12, n_models=1, n=3)):
        assert merge(**bad) == -1 and 'salsa_nn_tta_merge_multi' in _lib.last_error(), bad
    good = dict(a=p[0], x=p[1], files=2, n_chunks=6, len=8, hop=3, n_frames=23, C=12, fa=p[2], fx=p[3])

    def chunks(**kw):
        k = dict(good, **kw)
        return lib.salsa_nn_chunk_merge_multi(k['a'], k['x'], k['files'], k['n_chunks'], k['len'], k['hop'], k['n_frames'], k['C'], k['fa'],
                                              k['fx'], None)
    for bad in (dict(a=None), dict(x=None), dict(fa=None), dict(fx=None), dict(files=0), dict(n_chunks=0), dict(len=0), dict(hop=0),
                dict(n_frames=0), dict(C=0), dict(n_chunks=5), dict(n_chunks=7), dict(hop=9, n_chunks=3), dict(len=24, hop=24, n_chunks=2),
                dict(n_chunks=1), dict(n_chunks=2, len=30, hop=30), dict(files=1 << 20, C=100),
                dict(n_frames=1 << 24, len=1 << 24, hop=1, n_chunks=1, C=20)):
        assert chunks(**bad) == -1 and 'salsa_nn_chunk_merge_multi' in _lib.last_error(), bad


def test_device_wrappers_refuse_cpu_tensors_and_wrong_shapes():
    from salsa_amd.crnn.decode import chunk_merge_multi
    from salsa_amd.crnn.postprocess import combine_chunks_multi
    from salsa_amd.crnn.tta import tta_merge_multi
    with pytest.raises(ValueError, match='CUDA'):
        chunk_merge_multi(torch.zeros(1, 2, 5, 12), torch.zeros(1, 2, 5, 36), 5, 5, n_frames=10, n_classes=4)
    with pytest.raises(ValueError, match='not \\(files'):
        chunk_merge_multi(torch.zeros(1, 2, 5, 12), torch.zeros(1, 2, 5, 12), 5, 5, n_frames=10, n_classes=4)
    with pytest.raises(ValueError, match='expected 6 chunks'):
        combine_chunks_multi(np.zeros((7, 8, 12), F32), np.zeros((7, 8, 36), F32), 8, 3, 23, 4)
    with pytest.raises(ValueError):
        tta_merge_multi(torch.zeros(3, 2, 4, 36), 1, [0, 1], 'foa', 4)               # 3 slabs for N = 2
    with pytest.raises(ValueError):
        tta_merge_multi(torch.zeros(2, 2, 4, 12), 1, [0, 1], 'foa', 4)               # an xyz slab of one track
