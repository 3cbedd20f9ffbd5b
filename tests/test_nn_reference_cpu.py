"""CPU checks behind tests/test_nn_kernels_at_scale_gpu.py: the wide convolution's dispatch (which instantiation every bench
layer reaches, at the SALSA / lin maps and at the mel maps), the 64 -> 64 convolution's geometry, its weight-gradient index
tables against a numpy restatement of the padded layout, and the power of the float64 checker in tests/nn_reference.py -- it
must reject small, realistic kernel bugs.  No GPU calls."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import nn_reference as nr

MAX_XL_BYTES = 53248                    # conv_wide.hip: one input chunk's LDS buffer


@pytest.fixture(scope='module')
def lib():
    from salsa_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def wide_rows(tm, h, w):
    return (tm + w - 2) // w + 1 + 2 + (tm + h * w - 2) // (h * w) + 1


def wide_xl_bytes(tm, h, w):
    return (wide_rows(tm, h, w) * (w + 2) * 64 + 1023) & ~1023


def wide_tile(n, h, w, cout):
    """conv_wide.hip's wide_tile restated: (pixels per tile, output channels per tile)"""
    p = n * h * w
    big_ok = wide_xl_bytes(512, h, w) <= MAX_XL_BYTES
    if cout % 128 == 0 and big_ok and (p + 511) // 512 * (cout // 128) >= 192:
        return 512, 128
    if cout % 128 == 0 and (p + 255) // 256 * (cout // 128) >= 192:
        return 256, 128
    return (512 if big_ok and (p + 511) // 512 * (cout // 64) >= 192 else 256), 64


def config(lib, n, h, w, cout):
    tn = C.c_int(-7)
    tm = lib.salsa_nn_conv3x3_wide_config(n, h, w, cout, C.byref(tn))
    return tm, tn.value


def wrw3(h, w):
    """conv_wide.hip's wrw3_supported restated: three tile buffers when a tile's x slots are few enough"""
    rc, ic = (127 + w - 1) // w, (127 + h * w - 1) // (h * w)
    xs = (127 + 2 * rc + (w + 2) * ic + 2 * (w + 2) + 3 + 15) & ~15
    lds = 3 * (xs * 64 + 128 * 256) + 3 * ((xs + 63) // 64) * 256 + 5 * 512 + 256
    return (xs + 63) // 64 + 2 <= 8 and xs // 16 <= 24 and lds <= 160 * 1024


WRW_IMMEDIATE_W = (50, 25, 12)          # conv_wide.hip: widths with their own weight-gradient instantiation; others: W2C = 0


def c64_plan(n, h, w, th=4, tw=32):
    """conv_internal.h's c64_plan restated: (tiles, transposed) -- the map is handed over with its axes swapped when that needs
    fewer than 95 % of the tiles (TH x TW = 4 x 32 for the forward and the weight gradient alike)"""
    tn = n * -(-h // th) * -(-w // tw)
    tt = n * -(-w // th) * -(-h // tw)
    return (tt, 1) if tt * 100 < tn * 95 else (tn, 0)


def c64_config(lib, n, h, w):
    tr = C.c_int(-7)
    tiles = lib.salsa_nn_conv3x3_c64_config(n, h, w, C.byref(tr))
    return tiles, tr.value


# the wide 3x3 layers of the CRNN (stages 2 - 4) at the bench's map sizes: (Cin, Cout, H, W); the data gradient of each is a
# Cout -> Cin convolution at the same map.  BENCH_WIDE: 200 frequency bins in (SALSA, linspec*); MEL_WIDE: 128 (melspec*)
BENCH_WIDE = [(64, 128, 160, 50), (128, 128, 160, 50), (128, 256, 80, 25), (256, 256, 80, 25), (256, 512, 40, 12), (512, 512, 40, 12)]
MEL_WIDE = [(64, 128, 160, 32), (128, 128, 160, 32), (128, 256, 80, 16), (256, 256, 80, 16), (256, 512, 40, 8), (512, 512, 40, 8)]
# (C, H, W) of the four residual stages' BatchNorms at the mel maps (the first: the 64 -> 64 stage after the stem's pool)
MEL_STAGES = [(64, 320, 64), (128, 160, 32), (256, 80, 16), (512, 40, 8)]


def _assert_wide_dispatch(lib, layers):
    for n in (8, 16, 32):
        for cin, cout, h, w in layers:
            assert lib.salsa_nn_conv3x3_wide_supported(n, h, w, cin, cout)
            assert config(lib, n, h, w, cout) == wide_tile(n, h, w, cout), ('fwd', n, cin, cout, h, w)
            assert lib.salsa_nn_conv3x3_wide_supported(n, h, w, cout, cin)
            assert config(lib, n, h, w, cin) == wide_tile(n, h, w, cin), ('dgrad', n, cin, cout, h, w)
            tm, _ = config(lib, n, h, w, cout)
            assert lib.salsa_nn_conv3x3_wide_stats_blocks(n, h, w, cin, cout) == (n * h * w + tm - 1) // tm


def test_wide_dispatch_at_every_bench_layer(lib):
    _assert_wide_dispatch(lib, BENCH_WIDE)
    # what batch 32 runs: every one of the four instantiations is reached by a bench layer
    assert config(lib, 32, 160, 50, 128) == (512, 128)          # 64 -> 128, 128 -> 128 forward; 128 -> 128 data gradient
    assert config(lib, 32, 80, 25, 256) == (512, 128)           # 128 -> 256, 256 -> 256 forward; 256 -> 256 data gradient
    assert config(lib, 32, 40, 12, 512) == (256, 128)           # 256 -> 512, 512 -> 512 forward; 512 -> 512 data gradient
    assert config(lib, 32, 160, 50, 64) == (512, 64)            # data gradient of 64 -> 128
    assert config(lib, 32, 80, 25, 128) == (256, 128)           # data gradient of 128 -> 256
    assert config(lib, 32, 40, 12, 256) == (256, 64)            # data gradient of 256 -> 512
    # a 512-pixel tile at 160 x 50 needs exactly the whole LDS buffer
    assert wide_xl_bytes(512, 160, 50) == MAX_XL_BYTES
    assert config(lib, 0, 8, 8, 64)[0] == -1 and config(lib, 2, 8, 8, 96)[0] == -1
    assert lib.salsa_nn_conv3x3_wide_config(2, 8, 8, 64, None) == -1


def test_wide_dispatch_at_every_mel_layer(lib):
    """the 128-bin maps (160 x 32, 80 x 16, 40 x 8) reach instantiations the 200-bin maps do not reach with the same Cout"""
    _assert_wide_dispatch(lib, MEL_WIDE)
    assert config(lib, 32, 160, 32, 128) == (512, 128)          # 64 -> 128, 128 -> 128 forward; 128 -> 128 data gradient
    assert config(lib, 32, 80, 16, 256) == (256, 128)           # 128 -> 256, 256 -> 256 forward (80 x 25: (512, 128))
    assert config(lib, 32, 40, 8, 512) == (256, 64)             # 256 -> 512, 512 -> 512 forward: 8 column blocks of 64
    assert config(lib, 32, 160, 32, 64) == (512, 64)            # data gradient of 64 -> 128
    assert config(lib, 32, 80, 16, 128) == (256, 64)            # data gradient of 128 -> 256 (80 x 25: (256, 128))
    assert config(lib, 32, 40, 8, 256) == (256, 64)             # data gradient of 256 -> 512; 512 -> 512's too (40 x 12: (256, 128))
    # the weight gradients: every mel width takes the generic (W2C = 0) kernel on three tile buffers
    for cin, cout, h, w in MEL_WIDE:
        assert lib.salsa_nn_conv3x3_wide_wrw_supported(32, h, w, cin, cout), (cin, cout, h, w)
        assert wrw3(h, w) and w not in WRW_IMMEDIATE_W, (h, w)
    # the 1 x 1 shortcuts of the three stride-2 blocks: forward, data gradient, weight gradient
    for cin, cout, h, w in (MEL_WIDE[0], MEL_WIDE[2], MEL_WIDE[4]):
        M = 32 * h * w
        assert lib.salsa_nn_conv1x1_supported(M, cin, cout) and lib.salsa_nn_conv1x1_supported(M, cout, cin)
        assert lib.salsa_nn_conv1x1_wrw_supported(M, cin, cout)


def test_batchnorm_takes_every_mel_stage(lib):
    for n in (8, 16, 32):
        for c, h, w in MEL_STAGES:
            for dtype in (0, 1):
                assert lib.salsa_nn_bn_supported(dtype, n * h * w, c), (n, c, h, w, dtype)


def test_c64_geometry_query(lib):
    """salsa_nn_conv3x3_c64_config against the restated plan: 320 x 100 (SALSA / lin) runs transposed, 320 x 64 (mel) does not
    -- 5120 tiles either way, so the persistent loop walks ~10 tiles per workgroup in the untransposed geometry"""
    assert c64_config(lib, 32, 320, 100) == (8000, 1) == c64_plan(32, 320, 100)
    assert c64_config(lib, 32, 320, 64) == (5120, 0) == c64_plan(32, 320, 64)
    assert c64_plan(32, 320, 64, tw=4, th=32) == (5120, 0)     # (both orientations tie: no transpose on a tie)
    assert c64_config(lib, 32, 640, 200) == c64_plan(32, 640, 200)
    for n in (1, 3, 32):
        for h in (1, 2, 3, 4, 5, 7, 8, 31, 32, 33, 40, 64, 100, 127, 128, 160, 320, 640):
            for w in (1, 3, 4, 5, 8, 12, 16, 25, 31, 32, 33, 50, 64, 65, 100, 128, 200):
                assert c64_config(lib, n, h, w) == c64_plan(n, h, w), (n, h, w)
    tr = C.c_int(-7)
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8), (1 << 24, 64, 64)):
        assert lib.salsa_nn_conv3x3_c64_config(*bad, C.byref(tr)) == -1, bad
    assert lib.salsa_nn_conv3x3_c64_config(2, 8, 8, None) == -1


def test_wide_supported_and_tile_size_at_the_lds_limit(lib):
    """_supported is 'a 256-pixel tile's chunk fits'; 512-pixel tiles only where their chunk fits -- both at equality"""
    at_limit = []
    for h in (12, 25, 40, 50, 160):
        for w in range(1, 400):
            fits256 = wide_xl_bytes(256, h, w) <= MAX_XL_BYTES
            assert bool(lib.salsa_nn_conv3x3_wide_supported(32, h, w, 64, 128)) == fits256, (h, w)
            if wide_xl_bytes(512, h, w) == MAX_XL_BYTES:
                at_limit.append((h, w))
            if fits256:
                assert config(lib, 32, h, w, 128) == wide_tile(32, h, w, 128), (h, w)
                assert config(lib, 32, h, w, 64) == wide_tile(32, h, w, 64), (h, w)
    assert (160, 50) in at_limit
    assert config(lib, 32, 160, 51, 128)[0] == 256                              # one column more: 54 272 B, no 512-pixel tiles
    assert wide_xl_bytes(256, 40, 200) > MAX_XL_BYTES and not lib.salsa_nn_conv3x3_wide_supported(2, 40, 200, 128, 128)


def numpy_tables(n, h, w, tm=128):
    """the padded layout: virtual row v(n, h) = n (H + 1) + h + 1, slot = v (W + 2) + w + 1; per 128-pixel tile the first
    slot its taps touch and the number of slots up to its last pixel's last tap"""
    nn_, hh, ww = np.meshgrid(np.arange(n), np.arange(h), np.arange(w), indexing='ij')
    vpos = ((nn_ * (h + 1) + hh + 1) * (w + 2) + ww + 1).reshape(-1)
    inv = np.full((n * (h + 1) + 3) * (w + 2) + 16, -1, np.int64)
    inv[vpos] = np.arange(vpos.size)
    P = n * h * w
    first = vpos[np.arange(0, P, tm)] - (w + 3)
    last = vpos[np.minimum(np.arange(0, P, tm) + tm - 1, P - 1)]
    return vpos, inv, np.stack([first, last - first + w + 4], 1).reshape(-1)


@pytest.mark.parametrize('shape', [(32, 160, 50), (32, 80, 25), (32, 40, 12), (3, 30, 33), (1, 5, 7), (5, 3, 40), (2, 64, 1)])
def test_wide_wrw_tables_match_the_padded_layout(lib, shape):
    n, h, w = shape
    L = int(lib.salsa_nn_conv3x3_wide_table_len(n, h, w))
    T = int(lib.salsa_nn_conv3x3_wide_tile_count(n, h, w))
    assert T == math.ceil(n * h * w / 128)
    vpos, inv, tb = np.empty(n * h * w, np.int32), np.empty(L, np.int32), np.empty(2 * T, np.int32)
    rc = lib.salsa_nn_conv3x3_wide_tables(n, h, w, vpos.ctypes.data_as(C.c_void_p), inv.ctypes.data_as(C.c_void_p),
                                          tb.ctypes.data_as(C.c_void_p))
    assert rc == 0
    ev, ei, et = numpy_tables(n, h, w)
    assert L == ei.size
    np.testing.assert_array_equal(vpos, ev)
    np.testing.assert_array_equal(inv, ei)
    np.testing.assert_array_equal(tb, et)
    # every slot a tile's taps read lies inside its bounds and inside the table
    for t in range(T):
        p = np.arange(t * 128, min((t + 1) * 128, n * h * w))
        taps = (vpos[p][:, None] + np.array([dy * (w + 2) + dx for dy in (-1, 0, 1) for dx in (-1, 0, 1)])[None]).reshape(-1)
        assert taps.min() >= tb[2 * t] >= 0 and taps.max() < tb[2 * t] + tb[2 * t + 1] <= L


# ------------------------------------------------------------------------------------------------ the checker's power
def _bf16(t):
    return t.to(torch.bfloat16).double()


def _small_conv(seed=0, n=2, cin=64, cout=32, h=9, w=11):
    g = torch.Generator().manual_seed(seed)
    x = _bf16(torch.randn(n, cin, h, w, generator=g) + torch.linspace(-1, 2, cin).view(1, -1, 1, 1))   # offset channels
    wt = _bf16(torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5)
    return x, wt


def _fwd_check(y, ref, absum, cin):
    return nr.check(y, ref, nr.bf16_bound(ref, absum, nr.conv_accum_c(9 * cin)), 'conv')


def test_checker_accepts_a_correct_bf16_convolution():
    x, wt = _small_conv()
    ref, absum = nr.conv_fwd_ref(x, wt)
    y = _bf16(ref.float())                                          # float32 accumulation then one bf16 rounding
    assert _fwd_check(y, ref, absum, 64) <= 1
    assert torch.allclose(ref, torch.nn.functional.conv2d(x, wt, padding=1))


def test_checker_rejects_one_dropped_tap_at_a_border_pixel():
    x, wt = _small_conv(1)
    ref, absum = nr.conv_fwd_ref(x, wt)
    # pixel (image 1, row 0, last column): its taps reach the padding above and to the right; drop the one below-left
    n, h, w = 1, 0, x.shape[3] - 1
    bad = ref.clone()
    bad[n, :, h, w] -= (wt[:, :, 2, 0] * x[n, :, h + 1, w - 1][None]).sum(1)
    with pytest.raises(AssertionError):
        _fwd_check(_bf16(bad.float()), ref, absum, 64)


def test_checker_rejects_one_input_channel_missing_from_one_tap():
    x, wt = _small_conv(2)
    ref, absum = nr.conv_fwd_ref(x, wt)
    w2 = wt.clone()
    w2[:, 37, 1, 2] = 0                                              # channel 37 of the centre-right tap never read
    bad, _ = nr.conv_fwd_ref(x, w2)
    with pytest.raises(AssertionError):
        _fwd_check(_bf16(bad.float()), ref, absum, 64)


def test_checker_rejects_one_ulp_in_five_percent_of_a_bf16_output():
    x, wt = _small_conv(3)
    ref, absum = nr.conv_fwd_ref(x, wt)
    y = ref.float().to(torch.bfloat16)
    g = torch.Generator().manual_seed(3)
    pick = torch.rand(y.shape, generator=g) < 0.05
    up = torch.rand(y.shape, generator=g) < 0.5
    bits = y.view(torch.int16)
    bumped = torch.where(up, bits + 1, bits - 1).view(torch.bfloat16)   # one ulp away (same sign: magnitudes stay normal)
    y2 = torch.where(pick & (y != 0), bumped, y)
    with pytest.raises(AssertionError):
        _fwd_check(y2.double(), ref, absum, 64)


def test_checker_rejects_one_dropped_tile_in_a_bench_size_weight_gradient():
    """P = 32 x 160 x 50 = 256 000 pixels (stage 2); 8 -> 8 channels keep the CPU reference small, while c is the kernel's
    own chain at the bench layer 128 -> 128 (c = 209 u).  Losing the 128 pixels of one tile must fail the bound."""
    g = torch.Generator().manual_seed(4)
    n, h, w, cin, cout = 32, 160, 50, 8, 8
    x = _bf16(torch.randn(n, cin, h, w, generator=g) + 0.5)
    gy = _bf16(torch.randn(n, cout, h, w, generator=g))
    ref, absum = nr.conv_wgrad_ref(x, gy)
    c = nr.wide_wgrad_c(n, h, w, 128, 128)
    assert c == 209 * nr.U32
    assert nr.check(ref.float(), ref, c * absum, 'dW') < 1e-3
    t = 777                                                          # tile 777 = pixels 99 456 .. 99 583 (image 12)
    keep = torch.ones(n * h * w, dtype=torch.float64)
    keep[t * 128:(t + 1) * 128] = 0
    keep = keep.view(n, 1, h, w)
    bad, _ = nr.conv_wgrad_ref(x, gy * keep)
    with pytest.raises(AssertionError):
        nr.check(bad.float(), ref, c * absum, 'dW')
    # and the looser bound of a sequential float32 sum over every pixel would have let it through
    nr.check(bad.float(), ref, (n * h * w) * nr.U32 * absum, 'dW (sequential bound)')


def test_batchnorm_reference_matches_torch_batch_norm():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 16, 6, 5, generator=g, dtype=torch.float64) * 2 + torch.linspace(-3, 3, 16, dtype=torch.float64).view(1, -1, 1, 1)
    res = torch.randn(x.shape, generator=g, dtype=torch.float64)
    gamma = torch.rand(16, generator=g, dtype=torch.float64) + 0.5
    beta = torch.randn(16, generator=g, dtype=torch.float64)
    gy = torch.randn(4, 16, 3, 2, generator=g, dtype=torch.float64)
    for pool in (False, True):
        xa, ra, ga, ba = (t.clone().requires_grad_(True) for t in (x, res, gamma, beta))
        y = torch.relu(torch.nn.functional.batch_norm(xa, None, None, ga, ba, True, 0.1, 1e-5) + ra)
        y = torch.nn.functional.avg_pool2d(y, 2) if pool else y
        gyy = gy if pool else torch.randn(y.shape, generator=g, dtype=torch.float64)
        y.backward(gyy)
        r = nr.bn_train_ref(x, gamma, beta, 1e-5, residual=res, relu=True, pool=pool)
        b = nr.bn_bwd_ref(r, gamma, gyy, relu=True, pool=pool)
        assert torch.allclose(r['y'], y.detach())
        for k, t in (('dx', xa), ('dres', ra), ('dgamma', ga), ('dbeta', ba)):
            assert torch.allclose(b[k], t.grad, atol=1e-10), k


# ------------------------------------------------------------------------------------------------ the streamed reference
def _stream_case(seed, n=3, cin=16, cout=8, h=10, w=6):
    g = torch.Generator().manual_seed(seed)
    x = _bf16(torch.randn(n, cin, h, w, generator=g) + torch.linspace(-1, 2, cin).view(1, -1, 1, 1))
    wt = _bf16(torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5)
    shift = torch.randn(cout, generator=g)
    res = _bf16(torch.randn(n, cout, h, w, generator=g))
    return x, wt, shift, res


def _stream_check(y, x, wt, cin, pool=False, max_pix=24, **kw):
    """nr.check of y piece by piece against the streamed reference, as the GPU tests call it -> the maximum ratio"""
    c = nr.pooled_conv_c(9 * cin) if pool else nr.conv_accum_c(9 * cin)
    worst, rows = 0.0, 0
    for (n, a, b), ref, absum in nr.conv_fwd_ref_stream(x, wt, pool=pool, max_pix=max_pix, **kw):
        worst = max(worst, nr.check(y[n:n + 1, :, a:b], ref, nr.bf16_bound(ref, absum, c), 'clip %d rows %d:%d' % (n, a, b)))
        rows += b - a
    assert rows == y.shape[0] * y.shape[2]                            # every row of every clip exactly once
    return worst


def test_streamed_reference_equals_the_whole_batch_one_piece_by_piece():
    """bands of 4 (pooled: 4) rows cut through every clip of a ragged 3 x 9 x 11 map (and a 3 x 10 x 6 one, pooled): each
    piece equals conv_fwd_ref (+ F.avg_pool2d) on the same rows, with and without shift / residual / ReLU, and 1x1 filters"""
    g = torch.Generator().manual_seed(6)
    x = _bf16(torch.randn(3, 16, 9, 11, generator=g) + 0.5)
    wt = _bf16(torch.randn(8, 16, 3, 3, generator=g) * 0.1)
    shift, res = torch.randn(8, generator=g), _bf16(torch.randn(3, 8, 9, 11, generator=g))
    for kw in (dict(), dict(shift=shift, relu=True), dict(shift=shift, residual=res, relu=True), dict(residual=res)):
        ref, absum = nr.conv_fwd_ref(x, wt, **kw)
        pieces = list(nr.conv_fwd_ref_stream(x, wt, max_pix=44, **kw))
        assert [p[0] for p in pieces] == [(n, a, min(9, a + 4)) for n in range(3) for a in (0, 4, 8)]
        for (n, a, b), r, s in pieces:
            assert torch.allclose(r, ref[n:n + 1, :, a:b], rtol=1e-13, atol=1e-13) and torch.allclose(s, absum[n:n + 1, :, a:b], rtol=1e-13)
    w1 = _bf16(torch.randn(8, 16, 1, 1, generator=g))
    ref, absum = nr.conv_fwd_ref(x, w1, shift=shift)
    for (n, a, b), r, s in nr.conv_fwd_ref_stream(x, w1, shift=shift, max_pix=30):
        assert torch.allclose(r, ref[n:n + 1, :, a:b], rtol=1e-13, atol=1e-13) and torch.allclose(s, absum[n:n + 1, :, a:b], rtol=1e-13)
    x, wt, shift, res = _stream_case(7)
    ref, absum = nr.conv_fwd_ref(x, wt, shift=shift, residual=res, relu=True)
    ref, absum = torch.nn.functional.avg_pool2d(ref, 2), torch.nn.functional.avg_pool2d(absum, 2)
    pieces = list(nr.conv_fwd_ref_stream(x, wt, shift=shift, residual=res, relu=True, pool=True, max_pix=24))
    assert [p[0] for p in pieces] == [(n, a, min(5, a + 2)) for n in range(3) for a in (0, 2, 4)]      # 4 input rows = 2 pooled
    for (n, a, b), r, s in pieces:
        assert torch.allclose(r, ref[n:n + 1, :, a:b], rtol=1e-13, atol=1e-13) and torch.allclose(s, absum[n:n + 1, :, a:b], rtol=1e-13)
    assert nr.pooled_conv_c(576) == nr.conv_accum_c(576) + 2 * nr.U32


def test_streamed_checker_accepts_float32_evaluations():
    x, wt, shift, res = _stream_case(8)
    v = nr.conv_fwd_ref(x, wt, shift=shift, residual=res, relu=True)[0].float()        # the float32 value before the rounding
    assert _stream_check(_bf16(v), x, wt, 16, shift=shift, residual=res, relu=True) <= 1
    pooled = 0.25 * ((v[:, :, 0::2, 0::2] + v[:, :, 1::2, 0::2]) + (v[:, :, 0::2, 1::2] + v[:, :, 1::2, 1::2]))   # the kernel's order
    assert _stream_check(_bf16(pooled), x, wt, 16, pool=True, shift=shift, residual=res, relu=True) <= 1


def test_streamed_checker_rejects_a_tap_lost_or_bled_at_the_first_row_of_clip_1():
    x, wt, shift, res = _stream_case(9)
    ref, _ = nr.conv_fwd_ref(x, wt)
    assert _stream_check(_bf16(ref.float()), x, wt, 16) <= 1
    # (i) pixel (clip 1, row 0, column 2) loses the tap below-left
    bad = ref.clone()
    bad[1, :, 0, 2] -= (wt[:, :, 2, 0] * x[1, :, 1, 1][None]).sum(1)
    with pytest.raises(AssertionError):
        _stream_check(_bf16(bad.float()), x, wt, 16)
    # (ii) the batch walked as one tall image: clip 1's first row takes clip 0's last row for its upper halo instead of zeros
    bleed = ref.clone()
    up = torch.nn.functional.pad(x[0, :, -1], (1, 1))                                  # (Cin, W + 2)
    for s in range(3):
        bleed[1, :, 0, :] += wt[:, :, 0, s] @ up[:, s:s + x.shape[3]]
    with pytest.raises(AssertionError):
        _stream_check(_bf16(bleed.float()), x, wt, 16)


def test_streamed_checker_rejects_a_pool_of_bf16_rounded_pixels_on_five_percent():
    """the fused pool must average the float32 values and round once; rounding the four pixels first is what an unfused
    convolution + pool does, and on 5 % of the outputs it must not pass"""
    x, wt, shift, res = _stream_case(10, n=4, cin=64, cout=32, h=12, w=16)
    kw = dict(shift=shift, residual=res, relu=True)
    v = nr.conv_fwd_ref(x, wt, **kw)[0].float()
    pool = lambda t: 0.25 * ((t[:, :, 0::2, 0::2] + t[:, :, 1::2, 0::2]) + (t[:, :, 0::2, 1::2] + t[:, :, 1::2, 1::2]))
    good, early = _bf16(pool(v)), _bf16(pool(v.to(torch.bfloat16).float()))
    assert _stream_check(good, x, wt, 64, pool=True, max_pix=64, **kw) <= 1
    pick = torch.rand(good.shape, generator=torch.Generator().manual_seed(10)) < 0.05
    with pytest.raises(AssertionError):
        _stream_check(torch.where(pick, early, good), x, wt, 64, pool=True, max_pix=64, **kw)


def test_streamed_checker_rejects_a_residual_shifted_by_one_pixel():
    x, wt, shift, res = _stream_case(11)
    moved = torch.roll(res, 1, dims=3)                                                   # the residual of the pixel to the left
    for pool in (False, True):
        y = nr.conv_fwd_ref(x, wt, shift=shift, residual=moved, relu=True)[0].float()
        if pool:
            y = torch.nn.functional.avg_pool2d(y, 2)
        with pytest.raises(AssertionError):
            _stream_check(_bf16(y), x, wt, 16, pool=pool, shift=shift, residual=res, relu=True)


# ------------------------------------------------------------------------------------------------ the full-resolution maps
# (N, H, W) -> (tiles, transposed) of the largest 64 -> 64 launches: the stem's second convolution in training and the
# inference path of a 60-s clip; every one has >= 16384 tiles, i.e. the 1024-workgroup persistent grid
C64_FULL_RES = [((32, 640, 200), (32000, 1)), ((32, 640, 128), (20480, 0)),
                ((32, 4800, 200), (240000, 1)), ((32, 2400, 100), (60000, 1)),
                ((32, 4800, 128), (153600, 0)), ((32, 2400, 64), (38400, 0))]
# (N, H, W, Cout) of the wide layers at inference (200-bin and 128-bin features): all take 512-pixel tiles
WIDE_FULL_RES = [(32, 1200, 50, 128), (32, 600, 25, 256), (32, 300, 12, 512), (32, 1200, 32, 128), (32, 600, 16, 256), (32, 300, 8, 512)]


def test_c64_geometry_and_grid_at_the_full_resolution_maps(lib):
    for (n, h, w), geo in C64_FULL_RES:
        assert c64_config(lib, n, h, w) == geo == c64_plan(n, h, w), (n, h, w)
        assert geo[0] >= 16384 and lib.salsa_nn_conv3x3_c64_stats_blocks(n, h, w) == 1024, (n, h, w)
    # the residual stage of an 8-s chunk, where the kernel tests stopped: the 512-workgroup grid
    assert lib.salsa_nn_conv3x3_c64_stats_blocks(32, 320, 100) == 512 and lib.salsa_nn_conv3x3_c64_stats_blocks(32, 320, 64) == 512
    # the weight gradient plans with the same 4 x 32 tiles: 512 workgroups (tiles >= 16384) of 63 / 40 tiles each; c64_wgrad_c
    # counts the untransposed grid (70 at 640 x 200), an upper bound of the chain
    assert -(-c64_plan(32, 640, 200)[0] // 512) == 63 and -(-c64_plan(32, 640, 128)[0] // 512) == 40
    assert nr.c64_wgrad_c(32, 640, 200) == (70 * 8 + 16 + 512) * nr.U32 and nr.c64_wgrad_c(32, 640, 128) == (40 * 8 + 16 + 512) * nr.U32


def test_wide_dispatch_at_the_inference_maps(lib):
    for n, h, w, cout in WIDE_FULL_RES:
        assert config(lib, n, h, w, cout) == wide_tile(n, h, w, cout) == (512, 128), (n, h, w, cout)
        for cin in (cout // 2, cout):                                # the first and the second convolution of a block
            assert lib.salsa_nn_conv3x3_wide_supported(n, h, w, cin, cout), (n, h, w, cin, cout)
    assert config(lib, 32, 40, 12, 512) == (256, 128)                # (training's 40 x 12 does not reach 512-pixel tiles at W = 12)


def test_python_eligibility_agrees_with_the_library_at_the_pixel_limit(lib):
    """Conv3x3._hip_eligible / _stem_eligible take their size condition from nn_ops._c64_map_ok; the kernels refuse
    N H W >= INT32_MAX / 64 = 33 554 431 pixels.  Both sides of the limit, host only (nothing is allocated)."""
    from salsa_amd.crnn import nn_ops
    tr = C.c_int(0)
    for shape, ok in (((1, 33554430, 1), True), ((1, 33554431, 1), False), ((1, 33554432, 1), False), ((33554430, 1, 1), True),
                      ((31, 1801, 601), False), ((32, 4800, 200), True), ((35, 4800, 200), False), ((2, 8, 8), True), ((0, 8, 8), False)):
        n, h, w = shape
        assert (lib.salsa_nn_conv3x3_c64_config(n, h, w, C.byref(tr)) != -1) == ok, shape
        assert bool(nn_ops._c64_map_ok(n, h, w)) == ok, shape
        assert (lib.salsa_nn_conv3x3_c64_stats_blocks(n, h, w) > 0) == ok, shape
    assert 31 * 1801 * 601 == 33554431
