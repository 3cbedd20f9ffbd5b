"""GPU tests of track_merge='align' (DESIGN.md section 9u): salsa_nn_tta_merge_multi and salsa_nn_chunk_merge_multi through their C
entry points against the numpy restatement of tests/track_align_reference.py, bit for bit and between NaN-filled guard bands; the
python wrappers; and infer_pipelined with overlapping chunks and tta= together, decode='device' against decode='host' and against
the torch path of SALSA_HIP_TTA=0."""
import ctypes as C

import numpy as np
import pytest
import torch

import track_align_reference as ref

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
GUARD = 64
F32 = np.float32


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def guarded(n, dtype=torch.float32):
    """n elements between two guard bands; the whole buffer filled with NaN (float) or -7 (int)"""
    fill = float('nan') if dtype == torch.float32 else -7
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf):
    g = torch.cat([buf[:GUARD], buf[-GUARD:]])
    return bool(torch.isnan(g).all()) if buf.dtype == torch.float32 else bool((g == -7).all())


def same_bits(a, b):
    a = a.detach().cpu().numpy() if hasattr(a, 'detach') else np.asarray(a)
    b = b.detach().cpu().numpy() if hasattr(b, 'detach') else np.asarray(b)
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def launch_merge(slab, n_models, ids, kind, C_, with_perm=True):
    """one salsa_nn_tta_merge_multi launch on a device slab (N, B, L, 9 C) -> act, xyz, perm (guards checked)"""
    from salsa_amd import _lib
    N, B, L, _ = slab.shape
    bx, xo = guarded(B * L * 9 * C_)
    ba, ao = guarded(B * L * 3 * C_)
    bp, po = guarded(N * B * L * C_, torch.int32)
    rc = _lib.load().salsa_nn_tta_merge_multi(ptr(slab), n_models, (C.c_int * len(ids))(*ids), len(ids), ref.KIND[kind], B, L, C_, ptr(xo),
                                              ptr(ao), ptr(po) if with_perm else None, stream())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert guards_intact(bx) and guards_intact(ba) and guards_intact(bp)
    assert with_perm or bool((po == -7).all())
    return ao.view(B, L, 3 * C_), xo.view(B, L, 9 * C_), po.view(N, B, L, C_)


# N = 1, 2, 3 for every kind, and 2 models x 16 FOA variants
MERGE_CASES = [('foa', 1, [0]), ('foa', 2, [11]), ('foa', 1, [5, 0, 9]), ('mic', 1, [6]), ('mic', 1, [7, 2]), ('mic', 3, [5]),
               ('gcc', 1, [3]), ('gcc', 1, [0, 2]), ('gcc', 1, [1, 3, 2]), ('foa', 2, list(range(16)))]


@pytest.mark.parametrize('kind,n_models,ids', MERGE_CASES)
def test_tta_merge_multi_kernel_equals_the_restatement(kind, n_models, ids):
    """C = 13 and 14, L = 7 and 75: cell counts that are no multiple of a wave or a workgroup; B L C = 1: one thread; the built tie,
    one-ulp and NaN cells sit in the first cells of every slab that has room for them"""
    N = n_models * len(ids)
    for C_ in (1, 12, 13, 14):
        for B in (1, 3):
            for L in (1, 7, 75):
                slab = ref.near_slab(N, B, L, C_, seed=N + 10 * C_ + B + L)
                n_special = ref.plant_special(slab, ids, kind, C_, seed=7)
                assert n_special == min(8, B * L * C_)
                want_a, want_x, want_p = ref.merge(slab, n_models, ids, kind, C_)
                dev = torch.from_numpy(slab).to(DEV)
                a, x, p = launch_merge(dev, n_models, ids, kind, C_)
                case = (C_, B, L)
                assert same_bits(x, want_x) and same_bits(a, want_a) and np.array_equal(p.cpu().numpy(), want_p), case
                if L == 75:
                    assert N == 1 or C_ == 1 or len(set(want_p[1:].ravel().tolist())) == 6, case       # every candidate was chosen somewhere
                    a2, x2, _ = launch_merge(dev, n_models, ids, kind, C_, with_perm=False)  # a second run; no candidate output
                    assert same_bits(a2, a) and same_bits(x2, x), case
                    if B == 3:                                                               # a clip alone as inside its batch
                        a1, x1, p1 = launch_merge(dev[:, 1:2].contiguous(), n_models, ids, kind, C_)
                        assert same_bits(a1, a[1:2]) and same_bits(x1, x[1:2]) and torch.equal(p1, p[:, 1:2]), case


def test_tta_merge_multi_wrapper_and_planted_permutations():
    from salsa_amd.crnn import tta
    from salsa_amd.crnn.nn_ops import accdoa_sed
    assert tta.USE_HIP_TTA
    ids, C_ = list(range(16)), 12
    base = ref.planted_tracks((3, 75, C_), seed=11)
    rng = np.random.default_rng(12)
    plain, mixed, sigmas = [], [], []
    for k in range(32):
        cells = (base + rng.uniform(-0.01, 0.01, base.shape)).astype(F32)
        sh, sigma = ref.shuffled(cells, 13 + k)
        plain.append(ref.rows_of(ref.swap_cells(cells, 'foa', ids[k % 16])))
        mixed.append(ref.rows_of(ref.swap_cells(sh, 'foa', ids[k % 16])))
        sigmas.append(sigma)
    mixed, plain, sigma = np.stack(mixed), np.stack(plain), np.stack(sigmas)
    _, plain_x, _ = ref.merge(plain, 2, ids, 'foa', C_, align_tracks=False)
    want_x = ref.rows_of(np.take_along_axis(ref.cells_of(plain_x, C_), sigma[0][..., None], axis=-2))
    want_p = ref.cand_of(np.take_along_axis(np.argsort(sigma, axis=-1), np.broadcast_to(sigma[0], sigma.shape), axis=-1))
    act, xyz, perm = tta.tta_merge_multi(torch.from_numpy(mixed).to(DEV), 2, ids, 'foa', C_, return_perm=True)
    assert xyz.is_cuda and same_bits(xyz, want_x) and np.array_equal(perm.cpu().numpy(), want_p)
    assert same_bits(act, accdoa_sed(xyz, 3 * C_))
    two = tta.tta_merge_multi(torch.from_numpy(mixed).to(DEV), 2, ids, 'foa', C_)
    assert len(two) == 2 and same_bits(two[1], xyz)


CHUNK_CASES = [(23, 8, 3), (24, 8, 4), (20, 5, 5), (5, 8, 8), (24, 8, 3)]      # triple overlap; double; the reshape; one chunk, trimmed; a leftover chunk


def chunk_case(files, n_frames, chunk_len, hop, C_, seed):
    n = len(ref.starts_of(n_frames, chunk_len, hop))
    xyz = ref.random_slab(files, n, chunk_len, C_, seed).copy()
    if n > 1 and chunk_len > hop:                               # the built cells meet in the first overlap of file 0
        c0, c1 = ref.cells_of(xyz[0, 0], C_).copy(), ref.cells_of(xyz[0, 1], C_).copy()
        for j, (_, R, V, _) in enumerate(ref.special_cells(seed)[:C_ * (chunk_len - hop)]):
            f, c = divmod(j, C_)
            c0[hop + f, c], c1[f, c] = R, V
        xyz[0, 0], xyz[0, 1] = ref.rows_of(c0), ref.rows_of(c1)
    act = np.random.default_rng(seed + 1).uniform(0, 1, xyz.shape[:3] + (3 * C_,)).astype(F32)
    return act, xyz


def launch_chunks(act, xyz, chunk_len, hop, n_frames, C_):
    from salsa_amd import _lib
    files, n_chunks = act.shape[:2]
    ba, fa = guarded(files * n_frames * 3 * C_)
    bx, fx = guarded(files * n_frames * 9 * C_)
    rc = _lib.load().salsa_nn_chunk_merge_multi(ptr(act), ptr(xyz), files, n_chunks, chunk_len, hop, n_frames, C_, ptr(fa), ptr(fx), stream())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert guards_intact(ba) and guards_intact(bx)
    return fa.view(files, n_frames, 3 * C_), fx.view(files, n_frames, 9 * C_)


@pytest.mark.parametrize('n_frames,chunk_len,hop', CHUNK_CASES)
def test_chunk_merge_multi_kernel_equals_the_restatement(n_frames, chunk_len, hop):
    from salsa_amd.crnn.decode import chunk_merge_multi
    for C_ in (1, 12, 13):
        act, xyz = chunk_case(3, n_frames, chunk_len, hop, C_, seed=n_frames + C_)
        want = [ref.combine(act[f], xyz[f], chunk_len, hop, n_frames, C_) for f in range(3)]
        da, dx = torch.from_numpy(act).to(DEV), torch.from_numpy(xyz).to(DEV)
        fa, fx = launch_chunks(da, dx, chunk_len, hop, n_frames, C_)
        for f in range(3):
            assert same_bits(fa[f], want[f][0]) and same_bits(fx[f], want[f][1]), (C_, f)
        again = launch_chunks(da, dx, chunk_len, hop, n_frames, C_)
        alone = launch_chunks(da[1:2].contiguous(), dx[1:2].contiguous(), chunk_len, hop, n_frames, C_)
        assert same_bits(again[0], fa) and same_bits(again[1], fx) and same_bits(alone[0], fa[1:2]) and same_bits(alone[1], fx[1:2])
        wa, wx = chunk_merge_multi(da, dx, chunk_len, hop, n_frames=n_frames, n_classes=C_)          # the python wrapper
        assert same_bits(wa, fa) and same_bits(wx, fx)
        if hop == chunk_len or len(ref.starts_of(n_frames, chunk_len, hop)) == 1:                     # no arithmetic: the reshape
            assert same_bits(fa, act.reshape(3, -1, 3 * C_)[:, :n_frames]) and same_bits(fx, xyz.reshape(3, -1, 9 * C_)[:, :n_frames])
    with pytest.raises(ValueError, match='refused'):
        chunk_merge_multi(da, dx, chunk_len, hop, n_frames=n_frames + 40, n_classes=C_)


# ------------------------------------------------------------------------------------------------------------------ end to end
def sorted_rows(rows):
    return [sorted(map(tuple, r)) for r in rows]


def test_infer_pipelined_with_chunks_and_tta_device_host_and_torch_legs_agree(monkeypatch):
    """the stub forward of the CPU tests (exactly FOA-equivariant, bit-equal on chunks, tracks shuffled anew at every call) through
    overlapping chunks with a leftover one and all 16 FOA variants"""
    from salsa_amd.crnn import tta
    from salsa_amd.crnn.infer import infer_pipelined
    feats = (torch.randn(3, 7, 160, 8, generator=torch.Generator().manual_seed(4)) * 2).to(DEV)
    kw = dict(sub_batch=2, sed_threshold=0.35, n_label_frames=20, output_format='multi_accdoa', n_classes=2, eval_version='2020',
              unify_deg=0.001, chunk_len=64, chunk_hop_len=40, tta=('foa', 'salsa'), track_merge='align')
    run = lambda seed, decode: infer_pipelined(3, lambda lo, hi: feats[lo:hi], ref.stub_forward(2, shuffle_seed=seed), decode=decode, **kw)
    assert tta.USE_HIP_TTA
    device, host = run(9, 'device'), run(9, 'host')
    assert device == host and 60 < sum(len(r) for r in device) < 3 * 20 * 2 * 3
    assert sorted_rows(device) == sorted_rows(run(None, 'device'))                                  # the unshuffled stub's rows
    monkeypatch.setattr(tta, 'USE_HIP_TTA', False)                                                  # SALSA_HIP_TTA=0: the torch operators
    assert run(9, 'host') == host and run(9, 'device') == host


def test_multi_accdoa_trainer_infer_tta_merges_its_recorded_forwards():
    from salsa_amd.crnn.nn_ops import accdoa_sed
    from salsa_amd.crnn.train import Trainer
    torch.manual_seed(3)
    tr = Trainer(DEV, total_steps=10 ** 6, output_format='multi_accdoa', n_classes=2)
    x = torch.randn(2, 7, 160, 200, generator=torch.Generator().manual_seed(5)).to(DEV)
    with pytest.raises(ValueError, match='test-time augmentation'):
        tr.infer_tta(x, 'foa', variants=[0, 6, 9])
    outs, plain = [], tr.infer

    def recording(v):
        outs.append(tuple(t.clone() for t in plain(v)))
        return outs[-1]
    tr.infer, tr.track_merge = recording, 'align'
    act, xyz = tr.infer_tta(x, 'foa', variants=[0, 6, 9])
    assert len(outs) == 3 and act.shape == (2, 20, 6) and xyz.shape == (2, 20, 18)
    want_a, want_x, _ = ref.merge(np.stack([o[1].float().cpu().numpy() for o in outs]), 1, [0, 6, 9], 'foa', 2)
    assert same_bits(xyz, want_x) and same_bits(act, want_a) and same_bits(act, accdoa_sed(xyz, 6))
