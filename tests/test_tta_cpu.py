"""CPU tests of test-time augmentation and ensembling: the inverse target transform, the variant indexing,
the per-element arithmetic of salsa_nn_tta_variant / salsa_nn_tta_merge (salsa_amd/csrc/tta.h built with g++: tests/hostemu/
tta_emu.cpp) against the torch operators and the restatement of tests/tta_reference.py, TtaForward and the tta= keyword on toy
forwards, and the launchers' argument checks on the built library."""
import ctypes as C
import os
import subprocess

import pytest
import torch

import tta_reference as ref
from conftest import ROOT

KINDS = ('foa', 'mic', 'gcc')
MERGE_CASES = ref.MERGE_CASES


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('tta_emu') / 'libtta_emu.so')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-o', so,
                           os.path.join(ROOT, 'tests', 'hostemu', 'tta_emu.cpp')])
    L = C.CDLL(so)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    L.emu_variant_bits.argtypes = [C.c_int, C.c_int, ip]
    L.emu_variant.argtypes = [fp, C.c_int64, C.c_int64, fp] + [C.c_int] * 6
    L.emu_merge.argtypes = [fp, fp, C.c_int, ip] + [C.c_int] * 5 + [fp, fp]
    return L


def _fp(t):
    return C.cast(t.data_ptr(), C.POINTER(C.c_float))


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------------- 1. the inverse transform
@pytest.mark.parametrize('nc', [12, 14])
@pytest.mark.parametrize('kind', KINDS)
def test_unswap_is_the_inverse_of_the_swap_bit_for_bit(kind, nc):
    from salsa_amd.augment import swap_targets
    from salsa_amd.crnn.tta import unswap_targets, variant_bits
    fmt = 'foa' if kind == 'foa' else 'mic'
    y = ref.random_doa(3, 7, nc, seed=nc)
    assert (y == 0).any() and (y.view(torch.int32) == -2 ** 31).any() and (y.abs() == 1).any()     # +0, -0 and +-1 are in it
    seen = set()
    for v in range(ref.V[kind]):
        m = torch.tensor(variant_bits(kind, v)).expand(3, -1)
        s = swap_targets(y, m, fmt, nc)
        assert same_bits(unswap_targets(s, m, fmt, nc), y), v
        assert same_bits(swap_targets(unswap_targets(y, m, fmt, nc), m, fmt, nc), y), v
        assert same_bits(unswap_targets(y, m, fmt, nc), ref.unswap(y, kind, v, nc)), v
        seen.add(s.numpy().tobytes())
    assert len(seen) == ref.V[kind]                                    # the swaps are all different maps
    # per-sample bits: every sample of a batch gets its own pattern
    mb = torch.tensor([variant_bits(kind, v) for v in (1, ref.V[kind] - 1, 2)])
    s = swap_targets(y, mb, fmt, nc)
    assert same_bits(unswap_targets(s, mb, fmt, nc), y) and not same_bits(s, y)


# ---------------------------------------------------------------------------------------------------- 2. variant indexing
@pytest.mark.parametrize('kind', KINDS)
def test_variant_bits_enumerate_every_pattern_once(kind, emu):
    from salsa_amd.crnn.tta import n_variants, tta_variant, variant_bits
    V = n_variants(kind)
    assert V == ref.V[kind] == emu.emu_n_variants(ref.KIND[kind])
    pats = [variant_bits(kind, v) for v in range(V)]
    assert len(set(pats)) == V and pats[0] == (0,) * len(pats[0]) and pats == [tuple(ref.bits(kind, v)) for v in range(V)]
    if kind == 'gcc':
        assert sorted(pats) == sorted([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)])
    else:
        assert set(pats) == {tuple((i >> j) & 1 for j in range(len(pats[0]))) for i in range(2 ** len(pats[0]))}
    for v in range(V):                                                                             # the kernels' own statement
        m = (C.c_int * 4)(9, 9, 9, 9)
        emu.emu_variant_bits(ref.KIND[kind], v, m)
        assert tuple(m)[:len(pats[v])] == pats[v] and all(b == 0 for b in tuple(m)[len(pats[v]):])
    for v in (-1, V):
        with pytest.raises(ValueError):
            variant_bits(kind, v)
    x = torch.randn(2, ref.CHANNELS[kind], 4, 8)
    assert tta_variant(x, kind, 0) is x and tta_variant(x, kind, 0).data_ptr() == x.data_ptr()    # variant 0: no copy
    assert tta_variant(x, kind, 1).data_ptr() != x.data_ptr()


# ---------------------------------------------------------------------------------------------------- 3. the variant body
@pytest.mark.parametrize('kind,T,F', [('foa', 5, 200), ('mic', 5, 200), ('gcc', 5, 128), ('gcc', 5, 25), ('foa', 5, 25)])
def test_hostemu_variant_equals_the_torch_swaps(emu, kind, T, F):
    from salsa_amd.crnn.tta import tta_variant
    Cn = ref.CHANNELS[kind]
    g = torch.Generator().manual_seed(F + Cn)
    full = torch.randn(4, Cn, T + 3, F, generator=g)
    views = {'dense': full[:3, :, :T].contiguous(), 'time-cropped': full[:3, :, 2:2 + T], 'batch-strided': full[::2, :, 1:1 + T]}
    for name, x in views.items():
        B = x.shape[0]
        assert name == 'dense' or not x.is_contiguous()
        for v in range(ref.V[kind]):
            want = ref.variant(x, kind, v)
            assert same_bits(tta_variant(x, kind, v).contiguous(), want), (name, v)               # the CPU path of the product
            for width in (1, 4):
                out = torch.full((B, Cn, T, F), float('nan'))
                rc = emu.emu_variant(_fp(x), x.stride(0), x.stride(1), _fp(out), B, T, F, ref.KIND[kind], v, width)
                if width == 4 and (T * F) % 4:
                    assert rc == -2                                                                  # no 16-byte path for this shape
                    continue
                if width == 4 and rc == -2:                                                          # a view that starts off a 16-byte line
                    assert x.data_ptr() % 16 or x.stride(0) % 4 or x.stride(1) % 4 or (kind == 'gcc' and F % 4)
                    continue
                assert rc == 0 and same_bits(out, want), (name, v, width)
    if (T * F) % 4 == 0 and (kind != 'gcc' or F % 4 == 0):                                          # the wide body did run on the dense view
        out = torch.empty((3, Cn, T, F))
        x = views['dense']
        assert emu.emu_variant(_fp(x), x.stride(0), x.stride(1), _fp(out), 3, T, F, ref.KIND[kind], 1, 4) == 0


def test_mic_variants_with_several_bits_are_sequential_differences(emu):
    """x_v for a MIC variant with bits 1 and 2 set is NOT one closed-form permutation: the phase rows are re-referenced twice in
    float32, in the reference's order.  The body must round as the operator does, which a differently associated form does not."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 7, 4, 8, generator=g) * 3
    want = ref.variant(x, 'mic', 6)
    out = torch.empty_like(x)
    assert emu.emu_variant(_fp(x), x.stride(0), x.stride(1), _fp(out), 2, 4, 8, 2, 6, 1) == 0 and same_bits(out, want)
    closed = -x[:, 4]                                            # row 5 = c6' - c4' = (-c6) - (c4 - c6), which is -c4 only on paper
    assert not same_bits(closed, want[:, 5]) and torch.allclose(closed, want[:, 5], atol=1e-5)


# ---------------------------------------------------------------------------------------------------- 4, 5. the merge body
def emu_merge(emu, prob, xyz, n_models, ids, kind, nc):
    _, B, L, _ = prob.shape
    po, xo = torch.full((B, L, nc), float('nan')), torch.full((B, L, 3 * nc), float('nan'))
    rc = emu.emu_merge(_fp(prob), _fp(xyz), n_models, (C.c_int * len(ids))(*ids), len(ids), ref.KIND[kind], B, L, nc, _fp(po), _fp(xo))
    assert rc == 0
    return po, xo


@pytest.mark.parametrize('nc', [12, 14])
@pytest.mark.parametrize('kind,n_models,ids', MERGE_CASES)
def test_hostemu_merge_equals_the_restatement_and_float64(emu, kind, n_models, ids, nc):
    from salsa_amd.crnn.tta import tta_merge
    prob, xyz = ref.slab_case(kind, nc, n_models, ids)
    N = n_models * len(ids)
    assert prob.shape == (N, 3, 7, nc)
    want_p, want_d = ref.merge(list(prob), list(xyz), n_models, ids, kind, nc)
    got_p, got_d = emu_merge(emu, prob, xyz, n_models, ids, kind, nc)
    assert same_bits(got_p, want_p) and same_bits(got_d, want_d)
    cpu_p, cpu_d = tta_merge(prob, xyz, n_models, ids, kind, nc)                                    # the CPU path of the product
    assert same_bits(cpu_p, want_p) and same_bits(cpu_d, want_d)
    # against the float64 mean: each of the N - 1 additions rounds within 2^-24 of a partial sum of at most N max|input|, which the
    # division by N turns into (N - 1) 2^-24 max|input|; the division's own rounding adds 2^-24 max|input| -> N 2^-24 max|input|
    p64, d64 = ref.merge64(list(prob), list(xyz), n_models, ids, kind, nc)
    for got, exact, src in ((got_p, p64, prob), (got_d, d64, xyz)):
        err = float((got.double() - exact).abs().max())
        bound = N * 2.0 ** -24 * float(src.abs().max())
        print('merge %s N=%d nc=%d: max error %.3e, bound %.3e' % (kind, N, nc, err, bound))
        assert err <= bound


def test_merge_rotates_back_each_variant_by_its_own_bits(emu):
    """slabs that hold S_m(d) for one d merge to d: every un-swapped summand IS d, so only the N - 1 additions of equal values and
    the division round (N 2^-24 relative); a wrong direction for any one variant is an error of order |d|"""
    from salsa_amd.augment import swap_targets
    d = ref.random_doa(3, 7, 12, seed=5)
    for kind in KINDS:
        ids = list(range(ref.V[kind]))
        fmt = 'foa' if kind == 'foa' else 'mic'
        xyz = torch.stack([swap_targets(d, torch.tensor(ref.bits(kind, v)).expand(3, -1), fmt, 12) for v in ids])
        prob = torch.rand(1, 3, 7, 12).expand(len(ids), -1, -1, -1).contiguous()
        got_p, got_d = emu_merge(emu, prob, xyz, 1, ids, kind, 12)
        for got, want in ((got_d, d), (got_p, prob[0])):
            assert bool(((got - want).abs() <= len(ids) * 2.0 ** -24 * want.abs()).all()), kind


# ---------------------------------------------------------------------------------------------------- 6. the un-swap direction
def test_equivariant_forward_every_variant_rotates_back_to_the_plain_output():
    from salsa_amd.crnn.tta import TtaForward, tta_variant, unswap_targets, variant_bits
    x = torch.randn(3, 7, 160, 200, generator=torch.Generator().manual_seed(8))
    fwd = ref.equivariant_foa_forward()
    p0, d0 = fwd(x)
    assert p0.shape == (3, 20, 12) and d0.shape == (3, 20, 36)
    moved = 0
    for v in range(16):
        p, d = fwd(tta_variant(x, 'foa', v))
        m = torch.tensor(variant_bits('foa', v)).expand(3, -1)
        assert same_bits(p, p0) and same_bits(unswap_targets(d, m, 'foa', 12), d0), v
        moved += int(not same_bits(d, d0))
    assert moved == 15                                                                               # (the swaps do move the output)
    p, d = TtaForward(fwd, 'foa', 'salsa')(x)
    assert p.shape == p0.shape and d.shape == d0.shape and p.dtype == p0.dtype and d.dtype == d0.dtype
    for got, want in ((p, p0), (d, d0)):
        rel = float(((got - want).abs() / want.abs().clamp_min(1e-30)).max())
        print('equivariant forward: max relative error %.3e' % rel)
        assert rel <= 16 * 2.0 ** -24


# ---------------------------------------------------------------------------------------------------- 7. TtaForward
def _slab_order(outputs, n_models, nv):
    """recorded outputs come variant-major (a variant is formed once and fed to every model); the slabs are model-major"""
    return [outputs[vi * n_models + mi] for mi in range(n_models) for vi in range(nv)]


@pytest.mark.parametrize('kind,variants,ids', [('foa', 'all', list(range(16))), ('mic', [5, 0, 7], [5, 0, 7]), ('gcc', 'all', [0, 1, 2, 3])])
def test_ttaforward_with_two_models_equals_the_restatement(kind, variants, ids):
    from salsa_amd.crnn.tta import TtaForward
    fmt, ft = ('foa', 'salsa') if kind == 'foa' else ('mic', 'salsa') if kind == 'mic' else ('mic', 'melspecgcc')
    Cn = ref.CHANNELS[kind]
    x = torch.randn(3, Cn, 32, 16, generator=torch.Generator().manual_seed(9))
    ins, outs = [], []
    fwds = [ref.recording(ref.toy_forward(12, scale=s, channels=Cn), ins, outs) for s in (1.0, 0.6)]
    tf = TtaForward(fwds, fmt, ft, variants=variants)
    assert tf.variant_ids == ids and tf.kind == kind
    p, d = tf(x)
    assert len(ins) == 2 * len(ids)
    for r, xin in enumerate(ins):
        assert same_bits(xin, ref.variant(x, kind, ids[r // 2])), r
    rec = _slab_order(outs, 2, len(ids))
    want_p, want_d = ref.merge([o[0] for o in rec], [o[1] for o in rec], 2, ids, kind, 12)
    assert same_bits(p, want_p) and same_bits(d, want_d)
    # the buffers are kept: a second call (a smaller batch) allocates nothing new and gives the same rows for the same clips
    slabs = (tf._prob.data_ptr(), tf._xyz.data_ptr())
    p2, d2 = tf(x[:2])
    assert (tf._prob.data_ptr(), tf._xyz.data_ptr()) == slabs and same_bits(p2, want_p[:2]) and same_bits(d2, want_d[:2])


def test_ttaforward_without_variants_is_the_plain_mean_and_accdoa_takes_the_merged_length():
    from salsa_amd.crnn.nn_ops import accdoa_sed
    from salsa_amd.crnn.tta import TtaForward
    x = torch.randn(3, 7, 32, 16, generator=torch.Generator().manual_seed(10))
    f1, f2 = ref.toy_forward(12, scale=1.0), ref.toy_forward(12, scale=0.6)
    for variants in (None, ()):
        p, d = TtaForward([f1, f2], 'mic', 'salsa', variants=variants)(x)
        assert same_bits(p, (f1(x)[0] + f2(x)[0]) / 2) and same_bits(d, (f1(x)[1] + f2(x)[1]) / 2)
    p1, d1 = TtaForward(f1, 'foa', 'salsa', variants=None)(x)                                        # one model, identity: the forward
    assert same_bits(p1, f1(x)[0]) and same_bits(d1, f1(x)[1])
    tf = TtaForward([f1, f2], 'foa', 'salsa', output_format='accdoa')
    p, d = tf(x)
    plain = TtaForward([f1, f2], 'foa', 'salsa')(x)
    assert same_bits(d, plain[1]) and same_bits(p, accdoa_sed(d, 12)) and not same_bits(p, plain[0])
    reused = [torch.empty(3, 4, 12), torch.empty(3, 4, 36)]

    def in_place(xv):                                                                                # a forward that reuses its output storage
        pv, dv = f1(xv)
        reused[0].copy_(pv)
        reused[1].copy_(dv)
        return reused[0], reused[1]
    got = TtaForward(in_place, 'foa', 'salsa')(x)
    want = TtaForward(f1, 'foa', 'salsa')(x)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])


# ---------------------------------------------------------------------------------------------------- 8. the tta= keyword
@pytest.mark.parametrize('chunks', [None, (80, 40)])
def test_infer_pipelined_tta_keyword_equals_the_hand_wrapped_forward(chunks):
    from salsa_amd.crnn.infer import infer_pipelined
    from salsa_amd.crnn.tta import TtaForward
    feats = torch.randn(5, 7, 160, 16, generator=torch.Generator().manual_seed(11)) * 2
    fwd = ref.toy_forward(12, scale=2.0)
    kw = dict(sub_batch=2, sed_threshold=0.4, n_label_frames=20, decode='host')
    if chunks:
        kw.update(chunk_len=chunks[0], chunk_hop_len=chunks[1])
    rows = infer_pipelined(5, lambda lo, hi: feats[lo:hi], fwd, tta=('foa', 'salsa'), **kw)
    by_hand = infer_pipelined(5, lambda lo, hi: feats[lo:hi], TtaForward(fwd, 'foa', 'salsa'), **kw)
    ready = infer_pipelined(5, lambda lo, hi: feats[lo:hi], None, tta=TtaForward(fwd, 'foa', 'salsa'), **kw)
    plain = infer_pipelined(5, lambda lo, hi: feats[lo:hi], fwd, **kw)
    assert rows == by_hand == ready and sum(len(r) for r in rows) > 50 and rows != plain


def test_infer_pipelined_without_tta_hands_the_featurized_tensor_itself_to_forward():
    from salsa_amd.crnn.infer import infer_clips_sharded, infer_pipelined
    feats = torch.randn(4, 7, 160, 16, generator=torch.Generator().manual_seed(12))
    made, got = [], []

    def featurize(lo, hi):
        made.append(feats[lo:hi])
        return made[-1]

    def fwd(x):
        got.append(x)
        return ref.toy_forward(12)(x)
    for kw in (dict(), dict(tta=None)):
        made.clear(), got.clear()
        infer_pipelined(4, featurize, fwd, sub_batch=2, n_label_frames=20, **kw)
        assert len(got) == 2 and all(a is b for a, b in zip(made, got))
    names = ['c', 'a', 'b']
    out = infer_clips_sharded(names, lambda ns: feats[:len(ns)], ref.toy_forward(12, scale=2.0), sub_batch=2, n_label_frames=20,
                              sed_threshold=0.4, tta=('foa', 'salsa'))
    want = infer_pipelined(3, lambda lo, hi: feats[:hi - lo], ref.toy_forward(12, scale=2.0), sub_batch=2, n_label_frames=20,
                           sed_threshold=0.4, tta=('foa', 'salsa'))
    assert [out[n] for n in sorted(names)] == want


def test_validate_and_fit_take_the_tta_keyword():
    import inspect

    from salsa_amd.crnn import fit, train
    assert inspect.signature(fit.validate).parameters['tta'].default is None
    assert inspect.signature(fit.fit).parameters['tta'].default is None
    assert list(inspect.signature(train.Trainer.infer_tta).parameters) == ['self', 'x', 'audio_format', 'feature_type', 'variants']


# ---------------------------------------------------------------------------------------------------- 9. refusals
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
    assert 'salsa_nn_tta_variant' in _lib.NN_EXPORTS and 'salsa_nn_tta_merge' in _lib.NN_EXPORTS
    assert os.path.join(ROOT, 'salsa_amd', 'csrc', 'tta.hip') in _lib.build_command()
    a, b = C.c_void_p(0x10000), C.c_void_p(0x20000)
    good = dict(d_in=a, bs=7 * 1000, cs=1000, d_out=b, batch=2, T=5, F=200, kind=1, v=3)

    def variant(**kw):
        k = dict(good, **kw)
        return lib.salsa_nn_tta_variant(k['d_in'], k['bs'], k['cs'], k['d_out'], k['batch'], k['T'], k['F'], k['kind'], k['v'], None)
    for bad in (dict(kind=0), dict(kind=4), dict(kind=-1), dict(v=16), dict(v=-1), dict(kind=2, v=8), dict(kind=3, v=4), dict(d_in=None),
                dict(d_out=None), dict(d_out=a), dict(batch=0), dict(batch=65536), dict(T=0), dict(F=0), dict(cs=999), dict(bs=6999),
                dict(kind=3, bs=9999), dict(T=1 << 20, F=1 << 11, cs=1 << 31, bs=7 << 31)):
        assert variant(**bad) == -1 and 'salsa_nn_tta_variant' in _lib.last_error(), bad
    ids = (C.c_int * 3)(5, 0, 9)
    mgood = dict(p=a, x=b, n_models=2, ids=ids, n=3, kind=1, B=3, L=7, nc=14, po=C.c_void_p(0x30000), xo=C.c_void_p(0x40000))

    def merge(**kw):
        k = dict(mgood, **kw)
        return lib.salsa_nn_tta_merge(k['p'], k['x'], k['n_models'], k['ids'], k['n'], k['kind'], k['B'], k['L'], k['nc'], k['po'], k['xo'], None)
    for bad in (dict(kind=0), dict(kind=4), dict(ids=(C.c_int * 3)(5, 16, 9)), dict(ids=(C.c_int * 3)(5, -1, 9)), dict(kind=2),
                dict(kind=3), dict(n_models=0), dict(n=0), dict(n_models=-1), dict(n=17, ids=(C.c_int * 17)()), dict(p=None), dict(x=None),
                dict(ids=None), dict(po=None), dict(xo=None), dict(B=0), dict(L=0), dict(nc=0), dict(B=1 << 15, L=1 << 15, nc=12)):
        assert merge(**bad) == -1 and 'salsa_nn_tta_merge' in _lib.last_error(), bad


def test_python_surface_refuses_wrong_channels_and_unknown_recipes():
    from salsa_amd import augment
    from salsa_amd.crnn.tta import TtaForward, tta_merge, tta_variant
    fwd = ref.toy_forward(12)
    with pytest.raises(ValueError, match=r'\(B, 7, T, F\)'):
        TtaForward(fwd, 'foa', 'salsa')(torch.zeros(2, 10, 16, 8))
    with pytest.raises(ValueError, match=r'\(B, 10, T, F\)'):
        tta_variant(torch.zeros(2, 7, 16, 8), 'gcc', 1)
    for pair in (('foa', 'melspecgcc'), ('mic', 'salsa_lite'), ('ambi', 'salsa')):
        with pytest.raises(NotImplementedError) as e:
            TtaForward(fwd, *pair)
        with pytest.raises(NotImplementedError) as want:
            augment.recipe(*pair)
        assert str(e.value) == str(want.value)
    for variants in ([16], [-1], 'some', list(range(16)) + [0]):
        with pytest.raises(ValueError):
            TtaForward(fwd, 'foa', 'salsa', variants=variants)
    with pytest.raises(ValueError):
        TtaForward([], 'foa', 'salsa')
    with pytest.raises(ValueError):
        tta_merge(torch.zeros(3, 2, 4, 12), torch.zeros(3, 2, 4, 36), 1, [0, 1], 'foa', 12)       # 3 slabs for N = 2
