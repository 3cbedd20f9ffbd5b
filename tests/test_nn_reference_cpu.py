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
    """conv_mfma.hip's c64_plan restated: (tiles, transposed) -- the map is handed over with its axes swapped when that needs
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
