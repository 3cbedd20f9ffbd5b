"""GPU tests of the small kernels beside the hot path -- salsa_nn_seld_loss / _bwd, salsa_nn_colsum2, salsa_scaler_accumulate,
salsa_normalize_batch, salsa_to_freq_major -- each called through its C entry point at the shapes where its loops, tails and edges
change, and held to a host reference (tests/small_kernels_reference.py holds the inputs, the references and the bounds with their
derivations; tests/test_small_kernels_cpu.py shows on the same inputs that float32 arithmetic meets them).  Every output lives
inside a larger allocation with guard bands on both sides, which must come back bit-identical; so must the parts of a buffer the
kernel has no business in (channels >= n_sc).  Each test prints its worst error / bound."""
import ctypes as C

import numpy as np
import pytest
import torch

import small_kernels_reference as sk

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
GUARD = 4096                    # bytes on each side of an output (a whole row of the widest shape here fits)
GUARD_BYTE = 0xA5


class Guarded:
    """a device buffer holding `host` (any numpy array) between two guard bands of GUARD_BYTE"""

    def __init__(self, host):
        host = np.ascontiguousarray(host)
        self.shape, self.dtype, self.nbytes = host.shape, host.dtype, host.nbytes
        raw = np.full(2 * GUARD + self.nbytes, GUARD_BYTE, np.uint8)
        raw[GUARD:GUARD + self.nbytes] = host.reshape(-1).view(np.uint8)
        self.raw = torch.from_numpy(raw).to(DEV)
        assert self.raw.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return C.c_void_p(self.raw.data_ptr() + GUARD)

    def host(self):
        """-> the buffer's content; asserts that both guard bands are as they were"""
        torch.cuda.synchronize()
        raw = self.raw.cpu().numpy()
        assert (raw[:GUARD] == GUARD_BYTE).all(), 'written before the buffer'
        assert (raw[GUARD + self.nbytes:] == GUARD_BYTE).all(), 'written past the buffer'
        return raw[GUARD:GUARD + self.nbytes].view(self.dtype).reshape(self.shape).copy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def lib():
    from salsa_amd import _lib
    return _lib.load()


def show(what, r):
    print('%s: error / bound %s' % (what, ', '.join('%s %.3g' % kv for kv in sorted(r.items()))))


# ------------------------------------------------------------------------------------------------------------------- SELD loss
def seld_loss(inp, w):
    """one salsa_nn_seld_loss call on a NaN workspace -> (out3, g_logit, g_doa), guards checked"""
    t = {k: dev(v) for k, v in inp.items()}
    rows, nc = inp['sed_gt'].shape
    out3 = Guarded(np.full(3, np.nan, np.float32))
    gl = Guarded(np.full((rows, nc), np.nan, np.float32))
    gd = Guarded(np.full((rows, 3 * nc), np.nan, np.float32))
    ws = Guarded(np.full(192, np.nan, np.float64))                                # SALSA_SELD_LOSS_WS
    rc = lib().salsa_nn_seld_loss(ptr(t['logit']), ptr(t['doa']), ptr(t['sed_gt']), ptr(t['doa_gt']), rows, nc, w[0], w[1], out3.ptr,
                                  gl.ptr, gd.ptr, ws.ptr, stream())
    assert rc == 0
    ws.host()
    return out3.host(), gl.host(), gd.host()


@pytest.mark.parametrize('extreme', [False, True], ids=['randn', 'extreme'])
@pytest.mark.parametrize('mask', sk.SELD_MASKS)
@pytest.mark.parametrize('rows,nc', sk.SELD_SHAPES)
def test_seld_loss_against_float64(rows, nc, mask, extreme):
    """shapes x masks x (3 randn | 200 logits overwritten with 0, -0.0, +-16.7, +-30, +-88, +-104).  Measured on MI355X, worst over all
    72 cases, as a share of each bound: sed 13 %, doa_loss 8 %, loss 37 % (of 2 ulp), g_logit 40 %; g_doa bit-equal everywhere."""
    inp = sk.seld_inputs(rows, nc, mask, extreme)
    out = seld_loss(inp, sk.SELD_WEIGHTS)
    show('seld_loss (%d, %d) %s%s' % (rows, nc, mask, ' extreme' if extreme else ''), sk.check_seld(inp, sk.SELD_WEIGHTS, *out))
    again = seld_loss(inp, sk.SELD_WEIGHTS)
    assert all(sk.same_bits(a, b).all() for a, b in zip(out, again))              # fixed-order sums: bit-reproducible


@pytest.mark.parametrize('w', sk.BWD_WEIGHTS)
@pytest.mark.parametrize('rows,nc', sk.BWD_SHAPES)
def test_seld_loss_bwd_under_every_combination_of_incoming_gradients(rows, nc, w):
    """(3200, 12): na + nb = 153 600 elements, more than the 512 x 256 threads the launch is capped at.  Measured on MI355X: out_a
    50 %, out_b 73 % of the 2^-23 bound (two roundings of half an ulp each)."""
    a, b = sk.bwd_inputs(rows, nc)
    da, db = dev(a), dev(b)
    g = {k: dev(np.array([v], np.float32)) for k, v in sk.BWD_G.items()}
    worst = {}
    for present in sk.BWD_COMBOS:
        oa, ob = Guarded(np.full(a.shape, np.nan, np.float32)), Guarded(np.full(b.shape, np.nan, np.float32))
        gp = [ptr(g[k]) if p else None for k, p in zip(('g_loss', 'g_sed', 'g_doa'), present)]
        rc = lib().salsa_nn_seld_loss_bwd(ptr(da), a.size, ptr(db), b.size, gp[0], gp[1], gp[2], w[0], w[1], oa.ptr, ob.ptr,
                                          stream())
        assert rc == 0
        for k, v in sk.check_bwd(a, b, present, w, oa.host(), ob.host()).items():
            worst[k] = max(worst.get(k, 0.0), v)
    show('seld_loss_bwd (%d, %d) weights %s' % (rows, nc, w), worst)


# --------------------------------------------------------------------------------------------------------------------- colsum2
def colsum2(a, b, pre_a=None, pre_b=None):
    """one salsa_nn_colsum2 call into zero-filled (or pre-filled) outputs -> (out_a, out_b or None)"""
    Cn = a.shape[1]
    da, db = dev(a), None if b is None else dev(b)
    oa = Guarded(np.zeros(Cn, np.float32) if pre_a is None else pre_a)
    ob = None if b is None else Guarded(np.zeros(Cn, np.float32) if pre_b is None else pre_b)
    rc = lib().salsa_nn_colsum2(ptr(da), ptr(db), oa.ptr, None if ob is None else ob.ptr, a.shape[0], Cn, stream())
    assert rc == 0
    return oa.host(), None if ob is None else ob.host()


class deterministic:
    """nn_ops.set_deterministic(on) for the block, then back to the default (selected by the next differentiable forward), the way
    test_deterministic_mode_gives_bit_equal_weight_gradients restores it"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from salsa_amd.crnn import nn_ops
        nn_ops.set_deterministic(self.on, DEV)
        assert nn_ops.is_deterministic() == self.on
        if self.on:
            nn_ops._DET_WS[DEV].view(torch.float32).fill_(float('nan'))           # the slabs are never cleared: all that is read is written first

    def __exit__(self, *exc):
        from salsa_amd.crnn import nn_ops
        nn_ops._DET_USER[0] = None


@pytest.mark.parametrize('det', [False, True], ids=['atomic', 'deterministic'])
@pytest.mark.parametrize('M,Cn', sk.COLSUM_PAIRS)
def test_colsum2_against_float64(M, Cn, det):
    """one matrix (b = NULL) and two different ones, atomics and ordered slabs.  Measured on MI355X: at most 13 % of the bound."""
    a, b = sk.colsum_inputs(M, Cn, 0), sk.colsum_inputs(M, Cn, 1)
    with deterministic(det):
        one, none = colsum2(a, None)
        two_a, two_b = colsum2(a, b)
        swapped_b, _ = colsum2(b, None)
        again = colsum2(a, b) if det else None
    assert none is None
    r = {'a alone': sk.check_colsum(a, one)['colsum'], 'a of two': sk.check_colsum(a, two_a)['colsum'],
         'b of two': sk.check_colsum(b, two_b)['colsum'], 'b alone': sk.check_colsum(b, swapped_b)['colsum']}
    show('colsum2 (%d, %d) %s' % (M, Cn, 'deterministic' if det else 'atomic'), r)
    # out_b is the sum of b and not of a: the two matrices' sums are further apart than both bounds together
    gap = np.abs(sk.colsum64(a) - sk.colsum64(b))
    assert (gap > 2 * (sk.colsum_bound(a) + sk.colsum_bound(b))).any()
    if det:
        assert sk.same_bits(two_a, again[0]).all() and sk.same_bits(two_b, again[1]).all()       # slab order: bit-reproducible
        assert sk.same_bits(one, two_a).all() and sk.same_bits(swapped_b, two_b).all()           # the same sum, alone or as one of two


@pytest.mark.parametrize('det', [False, True], ids=['atomic', 'deterministic'])
def test_colsum2_adds_to_what_the_outputs_hold(det):
    """the header asks for zeroed outputs because the kernel ADDS: a known non-zero vector must come back increased by the sums"""
    M, Cn = 200, 65
    a, b = sk.colsum_inputs(M, Cn, 0), sk.colsum_inputs(M, Cn, 1)
    rng = np.random.RandomState(3)
    pre_a, pre_b = (10.0 * rng.randn(Cn)).astype(np.float32), (10.0 * rng.randn(Cn)).astype(np.float32)
    with deterministic(det):
        out_a, out_b = colsum2(a, b, pre_a, pre_b)
    show('colsum2 into non-zero outputs, %s' % ('deterministic' if det else 'atomic'),
         {'a': sk.check_colsum(a, out_a, pre_a)['colsum'], 'b': sk.check_colsum(b, out_b, pre_b)['colsum']})


# ----------------------------------------------------------------------------------------------------------- scaler / normalise
def scaler_accumulate(dfeat, shape, sums):
    B, Cn, T, F, n_sc = shape
    rc = lib().salsa_scaler_accumulate(ptr(dfeat), B, Cn, T, F, n_sc, sums.ptr, stream())
    assert rc == 0, rc


@pytest.mark.parametrize('shape', sk.SCALER_SHAPES)
def test_scaler_accumulate_against_float64(shape):
    """Measured on MI355X: the sums exact (the addends' 24-bit mantissas at one exponent fit float64), the sums of squares at
    0.04 % of the bound; scaler_finish's float32 mean at 5 % and std at 7 % of 1e-6 relative (float32 rounding of the result)."""
    from salsa_amd import extractor
    B, Cn, T, F, n_sc = shape
    feat = sk.scaler_inputs(*shape)
    dfeat = dev(feat)
    sums = Guarded(np.zeros((2, n_sc, F), np.float64))
    scaler_accumulate(dfeat, shape, sums)
    once = sums.host()
    r = sk.check_scaler(feat, n_sc, once)
    dsums = torch.from_numpy(once).to(DEV)
    mean, std = extractor.scaler_finish(dsums, B * T)
    assert mean.shape == (n_sc, 1, F) and std.shape == (n_sc, 1, F) and mean.dtype == torch.float32
    mean64, std64 = sk.scaler_finish64(feat, n_sc)
    for name, got, ref in (('mean', mean, mean64), ('std', std, std64)):
        err = np.abs(got.cpu().numpy()[:, 0].astype(np.float64) - ref)
        assert (err <= 1e-6 * np.abs(ref)).all(), (name, float(err.max()))
        r[name] = float((err[ref != 0] / (1e-6 * np.abs(ref[ref != 0]))).max()) if (ref != 0).any() else 0.0
    scaler_accumulate(dfeat, shape, sums)                                          # into the non-zero sums: it accumulates
    r.update({k + ' twice': v for k, v in sk.check_scaler(feat, n_sc, sums.host(), calls=2).items()})
    show('scaler_accumulate %s' % (shape,), r)


@pytest.mark.parametrize('shape', sk.NORMALIZE_SHAPES)
def test_normalize_batch_is_bit_equal_to_numpy_float32(shape):
    B, Cn, T, F, n_sc = shape
    feat, mean, std = sk.normalize_inputs(*shape)
    buf = Guarded(feat)
    dm, ds = dev(mean), dev(std)
    rc = lib().salsa_normalize_batch(buf.ptr, B, Cn, T, F, n_sc, ptr(dm), ptr(ds), stream())
    assert rc == 0, rc
    got, want = buf.host(), sk.normalize32(feat, mean, std, n_sc)
    bad = ~sk.same_bits(got[:, :n_sc], want[:, :n_sc])
    print('normalize_batch %s: %d of %d normalised values differ from numpy float32' % (shape, int(bad.sum()), bad.size))
    assert not bad.any(), np.argwhere(bad)[:5]
    assert (got[:, n_sc:].view(np.uint32) == feat[:, n_sc:].view(np.uint32)).all(), 'a channel >= n_sc was written'


# ---------------------------------------------------------------------------------------------------------------- to_freq_major
@pytest.mark.parametrize('rows,T,F', sk.TRANSPOSE_SHAPES)
def test_to_freq_major_is_bit_equal_to_numpy(rows, T, F):
    x = sk.transpose_inputs(rows, T, F)
    dx = dev(x)
    out = Guarded(sk.untouched_pattern(rows * F * T, np.float64).reshape(rows, F, T))
    rc = lib().salsa_to_freq_major(ptr(dx), rows, T, F, out.ptr, stream())
    assert rc == 0, rc
    got, want = out.host(), sk.to_freq_major64(x)
    bad = ~sk.same_bits(got, want)
    print('to_freq_major (%d, %d, %d): %d of %d differ' % (rows, T, F, int(bad.sum()), bad.size))
    assert not bad.any(), np.argwhere(bad)[:5]
