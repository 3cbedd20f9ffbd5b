"""CPU checks behind tests/test_nn_kernels_at_scale_gpu.py, _full_res_gpu.py and _lite_maps_gpu.py: the wide convolution's dispatch
(which instantiation every bench layer reaches, at the SALSA / lin maps, at the mel maps and at the odd-width SALSA-Lite / IPD
maps), the 64 -> 64 convolution's geometry, its weight-gradient index
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
            for w in (1, 3, 4, 5, 8, 11, 12, 16, 23, 25, 31, 32, 33, 47, 50, 64, 65, 95, 100, 128, 191, 200, 382):
                assert c64_config(lib, n, h, w) == c64_plan(n, h, w), (n, h, w)
    # the SALSA-Lite / IPD maps: 640 x 191 and 320 x 95 (n_fft 512) run untransposed -- every row ends in a 31-column partial tile
    # (191 = 5 x 32 + 31, 95 = 2 x 32 + 31) -- while 320 x 47 (n_fft 256) runs transposed
    assert c64_config(lib, 32, 640, 191) == (30720, 0) == c64_plan(32, 640, 191)
    assert c64_config(lib, 32, 320, 95) == (7680, 0) == c64_plan(32, 320, 95)
    assert c64_config(lib, 32, 320, 47) == (3840, 1) == c64_plan(32, 320, 47)
    assert 191 % 32 == 31 and 95 % 32 == 31
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


@pytest.mark.parametrize('shape', [(32, 160, 50), (32, 80, 25), (32, 40, 12), (3, 30, 33), (1, 5, 7), (5, 3, 40), (2, 64, 1),
                                   (32, 160, 47), (32, 80, 23), (32, 40, 11), (32, 160, 95)])        # (the last four: SALSA-Lite / IPD)
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


# ------------------------------------------------------------------------------------------------ the SALSA-Lite / IPD maps
# SALSA-Lite and SALSA-IPD keep the bins lower_bin .. cutoff_bin - 1 of the spectrum (salsa_bin_limits): F = 191 at n_fft 512,
# 382 at 1024, 95 at 256; full SALSA at n_fft 256 compresses to 100.  Every 2 x 2 pool halves the width rounding DOWN, so a
# Lite width is odd at every stage: (T = 640) 640 x 191, 320 x 95, 160 x 47, 80 x 23, 40 x 11.
LITE_F, LITE1024_F, LITE256_F, SALSA256_F = 191, 382, 95, 100
WIDE_CHANNELS = [(64, 128), (128, 128), (128, 256), (256, 256), (256, 512), (512, 512)]
WG_XL = 28672                           # conv_wide.hip: the weight gradient's input tile buffer (448 slots of 64 bytes)


def family_widths(f):
    """the frequency widths of the stem map and the four stages' maps: floor-halving"""
    return [f >> k for k in range(5)]


def wide_layers(f):
    """(Cin, Cout, H, W) of the six wide 3x3 layers (stages 2 - 4) for F = f frequency bins and 640 frames"""
    ws = family_widths(f)
    return [(cin, cout, 160 >> (i // 2), ws[2 + i // 2]) for i, (cin, cout) in enumerate(WIDE_CHANNELS)]


def stages(f):
    """(C, H, W) of the four residual stages' BatchNorms"""
    ws = family_widths(f)
    return [(64 << k, 320 >> k, ws[1 + k]) for k in range(4)]


LITE_WIDE, LITE1024_WIDE, LITE256_WIDE, SALSA256_WIDE = (wide_layers(f) for f in (LITE_F, LITE1024_F, LITE256_F, SALSA256_F))
LITE_STAGES, LITE1024_STAGES, LITE256_STAGES, SALSA256_STAGES = (stages(f) for f in (LITE_F, LITE1024_F, LITE256_F, SALSA256_F))
LITE_FAMILIES = {'lite512': LITE_F, 'lite1024': LITE1024_F, 'lite256': LITE256_F, 'salsa256': SALSA256_F}


def wide_wrw_ok(h, w):
    """salsa_nn_conv3x3_wide_wrw_supported's size condition restated: a 128-pixel tile's input rows fit the tile buffer"""
    return wide_rows(128, h, w) * (w + 2) * 64 <= WG_XL


def test_lite_map_lists_follow_the_extractor(lib):
    from salsa_amd.extractor import bin_limits
    from salsa_amd.torch_ops import output_shape
    for n_fft, f in ((512, LITE_F), (1024, LITE1024_F), (256, LITE256_F)):
        lo, _, cut = bin_limits(24000, n_fft, 50, 2000)
        assert cut - lo == f, (n_fft, lo, cut)
        for kind in ('salsa_lite', 'salsa_ipd'):
            assert output_shape(8 * 24000, 'mic', kind, 24000, n_fft, 300, 50, 2000) == (7, 641, f)
    assert output_shape(8 * 24000, 'mic', 'salsa', 24000, 256, 300, 50, 4000) == (7, 641, SALSA256_F)
    assert output_shape(8 * 24000, 'mic', 'salsa', 24000, 512, 300, 50, 4000) == (7, 641, 200)
    assert family_widths(191) == [191, 95, 47, 23, 11] and family_widths(382) == [382, 191, 95, 47, 23]
    assert family_widths(95) == [95, 47, 23, 11, 5] and family_widths(100) == [100, 50, 25, 12, 6]
    assert all(w % 2 for f in (191, 382, 95) for w in family_widths(f)[:5] if w != 382)       # odd at every stage (382: from stage 1 on)
    assert LITE_WIDE == [(64, 128, 160, 47), (128, 128, 160, 47), (128, 256, 80, 23), (256, 256, 80, 23), (256, 512, 40, 11), (512, 512, 40, 11)]
    assert LITE1024_WIDE[0] == (64, 128, 160, 95) and LITE1024_WIDE[2] == (128, 256, 80, 47) and LITE256_WIDE[4] == (256, 512, 40, 5)
    assert LITE_STAGES == [(64, 320, 95), (128, 160, 47), (256, 80, 23), (512, 40, 11)]
    assert wide_layers(200) == BENCH_WIDE and wide_layers(128) == MEL_WIDE and stages(128) == MEL_STAGES


# what batch 32 reaches at every wide layer of a family: [(forward instantiation, data-gradient instantiation)] in layer order
LITE_WIDE_INST = {
    'lite512': [((512, 128), (512, 64)), ((512, 128), (512, 128)), ((512, 128), (256, 128)), ((512, 128), (512, 128)),
                ((256, 128), (256, 64)), ((256, 128), (256, 128))],
    # 160 x 95: a 512-pixel tile's chunk needs 68 608 B > MAX_XL_BYTES, so (256, 128) where the other families run (512, 128);
    # 80 x 47 with 128 channels out (the data gradient of 128 -> 256): (512, 128), a pairing no 200- or 128-bin map reaches
    'lite1024': [((256, 128), (256, 64)), ((256, 128), (256, 128)), ((512, 128), (512, 128)), ((512, 128), (512, 128)),
                 ((512, 128), (256, 128)), ((512, 128), (512, 128))],
    'lite256': [((512, 128), (512, 64)), ((512, 128), (512, 128)), ((256, 128), (256, 64)), ((256, 128), (256, 128)),
                ((256, 64), (256, 64)), ((256, 64), (256, 64))],
    'salsa256': [((512, 128), (512, 64)), ((512, 128), (512, 128)), ((256, 128), (256, 64)), ((256, 128), (256, 128)),
                 ((256, 64), (256, 64)), ((256, 64), (256, 64))]}


@pytest.mark.parametrize('family', sorted(LITE_FAMILIES))
def test_wide_dispatch_at_every_lite_layer(lib, family):
    f = LITE_FAMILIES[family]
    layers = wide_layers(f)
    _assert_wide_dispatch(lib, layers)
    for (cin, cout, h, w), (fwd, dgrad) in zip(layers, LITE_WIDE_INST[family]):
        assert config(lib, 32, h, w, cout) == fwd == wide_tile(32, h, w, cout), (family, 'fwd', cin, cout, h, w)
        assert config(lib, 32, h, w, cin) == dgrad == wide_tile(32, h, w, cin), (family, 'dgrad', cin, cout, h, w)
        # the weight gradient.  Only full SALSA's widths 50 / 25 / 12 have an instantiation of their own (salsa256 meets 25 and
        # 12); every Lite width takes the generic (W2C = 0) kernel.  The kernel takes a map when a 128-pixel tile's input rows
        # fit its 28 672-byte tile buffer -- W <= 62 at these heights -- and then all of these maps run on three tile buffers
        # (wrw3).  160 x 95 does NOT fit (7 rows x 97 slots x 64 B = 43 456 B): salsa_nn_conv3x3_wide_wrw_supported refuses it,
        # the entry point returns -1 and _Conv3x3Wide.backward hands that weight gradient to torch.  wrw3(160, 95) is false as
        # well, but the two-buffer kernel is not what production runs there: nothing of the library is.
        ok = bool(lib.salsa_nn_conv3x3_wide_wrw_supported(32, h, w, cin, cout))
        assert ok == wide_wrw_ok(h, w) == (w <= 62), (family, cin, cout, h, w)
        assert ok == wrw3(h, w), (family, h, w)
        assert (w in WRW_IMMEDIATE_W) == (family == 'salsa256' and w in (25, 12)), (family, w)
    assert not wrw3(160, 95) and not wide_wrw_ok(160, 95) and wide_rows(128, 160, 95) * 97 * 64 == 43456
    assert [l for l in layers if not wide_wrw_ok(l[2], l[3])] == (layers[:2] if family == 'lite1024' else [])
    assert wide_xl_bytes(512, 160, 95) == 68608 > MAX_XL_BYTES
    # the 1 x 1 shortcuts of the three stride-2 blocks: forward, data gradient, weight gradient
    for cin, cout, h, w in (layers[0], layers[2], layers[4]):
        M = 32 * h * w
        assert lib.salsa_nn_conv1x1_supported(M, cin, cout) and lib.salsa_nn_conv1x1_supported(M, cout, cin)
        assert lib.salsa_nn_conv1x1_wrw_supported(M, cin, cout)


@pytest.mark.parametrize('family', sorted(LITE_FAMILIES))
def test_batchnorm_takes_every_lite_stage(lib, family):
    for n in (2, 8, 16, 32):
        for c, h, w in stages(LITE_FAMILIES[family]) + [(64, 640, LITE_FAMILIES[family])]:
            for dtype in (0, 1):
                assert lib.salsa_nn_bn_supported(dtype, n * h * w, c), (n, c, h, w, dtype)


# ------------------------------------------------------------------------------------------------ the GPU cases' batch sizes
def smallest_batch(answers):
    """the smallest N in 1 .. 32 at which answers(N) == answers(32): the host queries then pick for the test what they pick for
    the bench batch; 2 where they do not depend on N at all"""
    want = answers(32)
    n = min(k for k in range(1, 33) if answers(k) == want)
    assert all(answers(k) == want for k in range(n, 33)), n          # (and nothing changes between there and 32)
    return max(n, 2) if n == 1 else n


def wide_answers(lib, cin, cout, h, w):
    return lambda n: (config(lib, n, h, w, cout), config(lib, n, h, w, cin), bool(lib.salsa_nn_conv3x3_wide_supported(n, h, w, cin, cout)),
                      bool(lib.salsa_nn_conv3x3_wide_supported(n, h, w, cout, cin)),
                      bool(lib.salsa_nn_conv3x3_wide_wrw_supported(n, h, w, cin, cout)))


def c64_answers(lib, h, w):
    """the 64 -> 64 kernels' plan: transposed or not, the forward grid (salsa_nn_conv3x3_c64_stats_blocks: 512, or 1024 from
    16384 tiles up) and the weight gradient's grid as c64_wgrad_c restates it (128 / 256 / 512 workgroups)"""
    def grid(n):
        tiles, tr = c64_config(lib, n, h, w)
        return tr, lib.salsa_nn_conv3x3_c64_stats_blocks(n, h, w), 512 if tiles >= 16384 else 256 if tiles >= 4096 else 128 if tiles >= 128 else tiles
    return grid


# (Cin, Cout, H, W) -> N of the wide GPU cases: every LITE_WIDE layer and the three layers only another family reaches
LITE_GPU_WIDE = LITE_WIDE + [LITE1024_WIDE[0], LITE1024_WIDE[2], LITE256_WIDE[4]]
LITE_BATCH = {(64, 128, 160, 47): 14, (128, 128, 160, 47): 14, (128, 256, 80, 23): 27, (256, 256, 80, 23): 27, (256, 512, 40, 11): 28,
              (512, 512, 40, 11): 28, (64, 128, 160, 95): 4, (128, 256, 80, 47): 27, (256, 512, 40, 5): 2}
# (H, W) -> N of the 64 -> 64 cases: 320 x 95 (256-workgroup weight gradient from 4096 tiles), 640 x 191 (1024 / 512 grids from
# 16384 tiles), 320 x 47 (transposed); the 60-s inference maps: the smallest N on the 1024-workgroup grid
LITE_C64_BATCH = {(320, 95): 18, (640, 191): 18, (320, 47): 5, (4800, 191): 3, (2400, 95): 10}
LITE_STEM_BATCH = 3                     # 7 -> 64 at 640 x 191: salsa_nn_conv3x3_stem_stats_blocks reaches its 1024 rows


def test_lite_gpu_batches_answer_the_host_queries_as_batch_32_does(lib):
    assert set(LITE_BATCH) == set(LITE_GPU_WIDE)
    for layer, n in LITE_BATCH.items():
        assert smallest_batch(wide_answers(lib, *layer)) == n, layer
    for (h, w), n in LITE_C64_BATCH.items():
        assert smallest_batch(c64_answers(lib, h, w)) == n, (h, w)
    assert smallest_batch(lambda n: lib.salsa_nn_conv3x3_stem_stats_blocks(n, 640, 191)) == LITE_STEM_BATCH
    assert c64_answers(lib, 4800, 191)(3)[1] == 1024 == c64_answers(lib, 2400, 95)(10)[1]
    # nothing else the GPU cases ask depends on N: 2
    for cin, cout, h, w in (LITE_WIDE[0], LITE_WIDE[2], LITE_WIDE[4]):
        assert smallest_batch(lambda n: (lib.salsa_nn_conv1x1_supported(n * h * w, cin, cout), lib.salsa_nn_conv1x1_supported(n * h * w, cout, cin),
                                         lib.salsa_nn_conv1x1_wrw_supported(n * h * w, cin, cout))) == 2
    for c, h, w in LITE_STAGES + [(128, 159, 47)]:
        assert smallest_batch(lambda n: (lib.salsa_nn_bn_supported(0, n * h * w, c), lib.salsa_nn_bn_supported(1, n * h * w, c))) == 2


# ------------------------------------------------------------------------------------------------ the checker at an odd width
def test_checker_accepts_float32_evaluations_of_the_pool_gradient_and_the_any_order_bound():
    """avgpool_bwd_ref is exact in float32 and in bf16 (a division by 4); a float32 evaluation of a weight gradient in torch's
    own summation order stays inside any_order_wgrad_bound"""
    g = torch.Generator().manual_seed(12)
    gy = torch.randn(2, 8, 4, 5, generator=g).to(torch.bfloat16)
    ref = nr.avgpool_bwd_ref(gy, 9, 11)
    assert ref.shape == (2, 8, 9, 11) and torch.equal(ref.to(torch.bfloat16).double(), ref) and torch.equal(ref.float().double(), ref)
    assert not bool(ref[:, :, 8].any()) and not bool(ref[:, :, :, 10].any())
    x = torch.randn(2, 8, 9, 11, generator=g, dtype=torch.float64).requires_grad_(True)
    torch.nn.functional.avg_pool2d(x, 2).backward(gy.double())
    assert torch.equal(x.grad, ref)
    nr.assert_dropped_plus_zero(ref.to(torch.bfloat16), 'bf16')
    nr.assert_dropped_plus_zero(ref.float(), 'float32')
    xq, wt = _small_conv(13, n=4, cin=16, cout=8, h=9, w=11)
    gyq = _bf16(torch.randn(4, 8, 9, 11, generator=g))
    wref, wabs = nr.conv_wgrad_ref(xq, gyq)
    w32 = torch.nn.grad.conv2d_weight(xq.float(), (8, 16, 3, 3), gyq.float(), padding=1)
    assert nr.check(_bf16(w32), wref, nr.any_order_wgrad_bound(wref, wabs, 4 * 9 * 11), 'dW') <= 1
    with pytest.raises(AssertionError):                                  # and it is no free pass: one pixel's products missing
        keep = torch.ones(4, 1, 9, 11, dtype=torch.float64)
        keep[2, 0, 8, 10] = 0
        nr.check(_bf16(nr.conv_wgrad_ref(xq, gyq * keep)[0].float()), wref, nr.any_order_wgrad_bound(wref, wabs, 4 * 9 * 11), 'dW')


def test_checker_accepts_a_float32_evaluation_of_the_eval_batchnorm():
    """bn_eval_ref against torch's eval-mode batch_norm, and the kernel's float32 statement order inside 16 u absum (+ bf16)"""
    g = torch.Generator().manual_seed(16)
    x = _bf16(torch.randn(2, 16, 9, 11, generator=g) * 2 + torch.linspace(-3, 3, 16).view(1, -1, 1, 1)).float()
    res = _bf16(torch.randn(2, 16, 9, 11, generator=g)).float()
    gamma, beta = torch.rand(16, generator=g) + 0.5, torch.randn(16, generator=g)
    rm, rv = torch.randn(16, generator=g), torch.rand(16, generator=g) + 0.5
    invstd = torch.rsqrt(rv + 1e-5)
    ref, absum = nr.bn_eval_ref(x, gamma, beta, rm, invstd, residual=res, relu=True)
    want = torch.relu(torch.nn.functional.batch_norm(x.double(), rm.double(), rv.double(), gamma.double(), beta.double(), False, 0.1, 1e-5)
                      + res.double())
    assert torch.allclose(ref, want, rtol=1e-6, atol=1e-6)               # (invstd is float32 in ref, float64 in torch's)
    v = lambda t: t.view(1, -1, 1, 1)
    y32 = torch.relu(((x - v(rm)) * v(invstd)) * v(gamma) + v(beta) + res)
    assert nr.check(y32, ref, 16 * nr.U32 * absum, 'bn eval fp32') <= 5 / 16 + 1e-3
    assert nr.check(_bf16(y32), ref, 16 * nr.U32 * absum + nr.BF16_REL * ref.abs(), 'bn eval bf16') <= 1
    with pytest.raises(AssertionError):                                  # the residual of the pixel to the left
        bad = torch.relu(((x - v(rm)) * v(invstd)) * v(gamma) + v(beta) + torch.roll(res, 1, dims=3))
        nr.check(_bf16(bad), ref, 16 * nr.U32 * absum + nr.BF16_REL * ref.abs(), 'bn eval bf16')


def test_checker_rejects_a_dropped_column_gradient_left_unwritten():
    """a pool backward over a 9 x 11 map that never stores the column (and row) the pool drops: in a NaN-filled buffer those
    elements stay NaN, in a recycled one they hold stale values or -0.0 -- none of them may pass"""
    g = torch.Generator().manual_seed(14)
    gy = torch.randn(2, 8, 4, 5, generator=g).to(torch.bfloat16)
    ref = nr.avgpool_bwd_ref(gy, 9, 11)
    good = ref.to(torch.bfloat16)
    assert nr.check(good, ref, 0 * ref, 'pool bwd') == 0
    nr.assert_dropped_plus_zero(good, 'pool bwd')
    for stale in (float('nan'), -0.0, 2.0 ** -20):
        for cut in ((slice(None), slice(10, 11)), (slice(8, 9), slice(None))):       # the last column / the last row
            bad = good.clone()
            bad[:, :, cut[0], cut[1]] = stale
            with pytest.raises(AssertionError):
                nr.assert_dropped_plus_zero(bad, 'pool bwd')
            if stale != 0:                                                           # (-0.0 == +0.0 to the value checker)
                with pytest.raises(AssertionError):
                    nr.check(bad, ref, 0 * ref, 'pool bwd')
    # the BatchNorm + pool backward's dres at the same map, against bn_bwd_ref's own bound
    x = torch.randn(2, 8, 9, 11, generator=g) + 0.5
    res = torch.randn(2, 8, 9, 11, generator=g)
    r = nr.bn_train_ref(x, torch.ones(8), torch.zeros(8), 1e-5, residual=res, relu=True, pool=True)
    b = nr.bn_bwd_ref(r, torch.ones(8), gy, relu=True, pool=True, bf16=True)
    assert not bool(b['dres'][:, :, :, 10].any()) and not bool(b['dres'][:, :, 8].any())
    dres = b['dres'].to(torch.bfloat16)
    keep = ~b['exempt']
    assert nr.check(dres.double()[keep], b['dres'][keep], b['b_dres'][keep], 'dres') <= 1
    dres[:, :, :, 10] = float('nan')
    with pytest.raises(AssertionError):
        nr.check(dres.double()[keep], b['dres'][keep], b['b_dres'][keep], 'dres')


def test_checker_rejects_a_partial_tile_whose_last_column_reads_the_next_row():
    """W = 47 = 32 + 15: the second tile of a row is partial.  A kernel that walks the map as one run of pixels takes, for the
    right-hand taps of the row's LAST column, the first pixel of the next row where the padding's zero belongs."""
    x, wt = _small_conv(15, n=2, cin=64, cout=32, h=5, w=47)
    ref, absum = nr.conv_fwd_ref(x, wt)
    assert _fwd_check(_bf16(ref.float()), ref, absum, 64) <= 1
    n, h, w = x.shape[0], x.shape[2], x.shape[3]
    bad = ref.clone()
    flat = torch.nn.functional.pad(x, (0, 0, 1, 2)).reshape(n, 64, -1)               # rows -1 .. h + 1, one after the other
    for r in range(3):                                                               # tap (r, 2) of pixel (hh, w - 1): row hh + r - 1, column w
        for hh in range(h):
            bad[:, :, hh, w - 1] += flat[:, :, (hh + r) * w + w] @ wt[:, :, r, 2].T
    assert torch.equal(bad[:, :, :, :w - 1], ref[:, :, :, :w - 1])
    with pytest.raises(AssertionError):
        _fwd_check(_bf16(bad.float()), ref, absum, 64)
    # one image, one row, one tap is enough
    one = ref.clone()
    one[1, :, 2, w - 1] += wt[:, :, 1, 2] @ x[1, :, 3, 0]
    with pytest.raises(AssertionError):
        _fwd_check(_bf16(one.float()), ref, absum, 64)
