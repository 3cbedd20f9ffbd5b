"""The CRNN's hand-written kernels at the SALSA-Lite / SALSA-IPD maps, against float64 references with the per-element bounds of
tests/nn_reference.py.  The Lite extractor keeps 191 frequency bins at n_fft 512 (382 at 1024, 95 at 256), and every 2 x 2 pool
halves an odd width rounding down, so the maps are 640 x 191, 320 x 95, 160 x 47, 80 x 23, 40 x 11: odd at every stage, which
neither the 200-bin nor the 128-bin family of tests/test_nn_kernels_at_scale_gpu.py and _full_res_gpu.py is anywhere.  Same
conventions as those files: inputs from _act / _filt, every case first asserts the instantiation it reaches (restated on the
CPU in tests/test_nn_reference_cpu.py), _report prints max err / bound.  Here every entry point is called directly: outputs
and gradient buffers are filled with NaN beforehand and lie between NaN guard bands, so an element left unwritten or a store
past the end fails.  Run alone:  python -m pytest -m gpu tests/test_nn_kernels_lite_maps_gpu.py -q -s

  kernel                    what only these maps reach
  64 -> 64 (c64)            640 x 191 and 320 x 95 UNtransposed with a 31-column partial tile at the end of every row (191 = 5 x 32
                            + 31); 320 x 47 (n_fft 256) transposed
  2 x 2 pools               every pool drops a last column: the stand-alone pool and BatchNorm + ReLU + pool, forward and backward
                            (the dropped column's gradient is +0.0); in eval mode the stem's pool is NOT fused (odd W)
  wide forward              160 x 95 (n_fft 1024): no 512-pixel tile fits, batch 32 runs (256, 128)
  wide data gradient        80 x 47 with 128 channels out: (512, 128)
  wide weight gradient      the generic (W2C = 0) kernel at every width; 160 x 95 is REFUSED (its tile buffer holds W <= 62) and
                            goes to torch: that fallback is tested here against float64 as well
  frequency mean / pools    11, 23 and 5 bins

The batch of a case is the smallest N at which the library's host queries answer as they do at N = 32 (LITE_BATCH,
LITE_C64_BATCH in test_nn_reference_cpu.py), 2 where they do not depend on N.  The whole model at 191 and 382 bins is at the end.
Wall time on one MI355X: 87 s for the 141 cases (profiles/nn_lite_maps_pytest_gpu.log, with the printed table).  The 137 kernel
cases take 16 s, none more than 4 s.  70 s go to the torch-layer legs of two whole-model comparisons, where MIOpen searches
maps it has not met before (46 s at 8 x 640 x 191, 23 s at 2 x 640 x 382; test_whole_model_hip_layers_on_vs_off itself spends
23 s that way at 200 bins); the on-the-fly case at 191 bins reuses the first one's maps and takes 0.6 s.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nn_reference as nr
from test_nn_kernels_at_scale_gpu import CL, DEV, _act, _features, _filt, _lib, _report
from test_nn_reference_cpu import (LITE1024_WIDE, LITE256_WIDE, LITE_BATCH, LITE_C64_BATCH, LITE_GPU_WIDE, LITE_STAGES, LITE_STEM_BATCH,
                                   LITE_WIDE, WRW_IMMEDIATE_W, c64_config, c64_plan, config, wide_tile, wide_wrw_ok, wrw3)

pytestmark = pytest.mark.gpu

PAD = 4096                               # guard elements before and after every buffer a kernel writes


def _ops():
    from salsa_amd.crnn import nn_ops
    return nn_ops


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def S():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _guarded(shape, dtype=torch.bfloat16):
    """-> (buffer, view): a NaN-filled buffer with PAD guard elements on either side of an (N, C, H, W) channels-last view, NaN too"""
    N, Cn, H, W = shape
    n = N * Cn * H * W
    buf = torch.full((n + 2 * PAD,), float('nan'), dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + n].view(N, H, W, Cn).permute(0, 3, 1, 2)


def _guarded_dw(shape):
    """-> (buffer, view): a float32 weight gradient of `shape` (contiguous) between NaN guards, zeroed: the kernels add to it"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), float('nan'), dtype=torch.float32, device=DEV)
    buf[PAD:PAD + n].zero_()
    return buf, buf[PAD:PAD + n].view(shape)


def _intact(buf, view, what):
    """no guard element changed, every element inside was written (none is NaN any more)"""
    n = view.numel()
    assert bool(torch.isnan(buf[:PAD]).all()) and bool(torch.isnan(buf[PAD + n:]).all()), what + ': a guard element changed'
    assert not bool(torch.isnan(buf[PAD:PAD + n]).any()), what + ': an element was not written (or is NaN)'


def _stream_check(what, y, x, w, c, **kw):
    """y against the streamed float64 reference, every piece of every clip (as tests/test_nn_kernels_full_res_gpu.py)"""
    worst, rows = 0.0, 0
    for (n, a, b), ref, absum in nr.conv_fwd_ref_stream(x, w, **kw):
        worst = max(worst, nr.check(y[n:n + 1, :, a:b], ref, nr.bf16_bound(ref, absum, c), '%s, clip %d rows %d:%d' % (what, n, a, b)))
        rows += b - a
        del ref, absum
    assert rows == y.shape[0] * y.shape[2]
    return _report(what, worst)


# --------------------------------------------------------------------------------------------- 64 -> 64
def _c64_call(x, wt, shift=None, res=None, relu=0, part=None):
    """salsa_nn_conv3x3_c64 / _stats / _bias_act into a guarded NaN-filled output"""
    L = _lib()
    n, _, h, w = x.shape
    buf, y = _guarded((n, 64, h, w))
    with torch.cuda.device(DEV):
        if part is not None:
            rc = L.salsa_nn_conv3x3_c64_stats(P(x), P(wt), P(y), P(part), n, h, w, S())
        elif shift is None:
            rc = L.salsa_nn_conv3x3_c64(P(x), P(wt), P(y), n, h, w, S())
        else:
            rc = L.salsa_nn_conv3x3_c64_bias_act(P(x), P(wt), P(shift), P(res), P(y), relu, n, h, w, S())
    assert rc == 0
    torch.cuda.synchronize()
    return buf, y


def _c64_case(n, h, w, seed):
    """forward, statistics epilogue, folded epilogue, data gradient and weight gradient (atomic and deterministic) of one map"""
    nn_ops = _ops()
    L = _lib()
    tiles, tr = c64_config(L, n, h, w)
    assert (tiles, tr) == c64_plan(n, h, w)
    blocks = L.salsa_nn_conv3x3_c64_stats_blocks(n, h, w)
    assert blocks == (1024 if tiles >= 16384 else 512 if tiles >= 512 else tiles)
    tag = '%dx%dx%d %s, %d tiles / %d' % (n, h, w, 'transposed' if tr else 'untransposed', tiles, blocks)
    x, gy, wt = _act(n, 64, h, w, seed), _act(n, 64, h, w, seed + 1, offset=False), _filt(64, 64, 3, seed + 2)
    c = nr.conv_accum_c(9 * 64)
    buf, y = _c64_call(x, wt)
    _intact(buf, y, 'c64 fwd ' + tag)
    _stream_check('c64 fwd ' + tag, y, x, wt, c)
    # training: the same output, and float64 partial sums of it per workgroup.  A sum's float32 chain: a row pair (1), two DPP
    # steps (2), the lane's running sum over the workgroup's ceil(tiles / blocks) tiles, three shuffles (3), + 2 spare
    part = torch.full((blocks, 2, 64), float('nan'), dtype=torch.float64, device=DEV)
    bufs, ys = _c64_call(x, wt, part=part)
    _intact(bufs, ys, 'c64 stats ' + tag)
    assert torch.equal(ys, y)
    del bufs, ys
    yd = y.double()
    c_s = (-(-tiles // blocks) + 8) * nr.U32
    _report('c64 stats sum ' + tag, nr.check(part[:, 0].sum(0), yd.sum(dim=(0, 2, 3)), c_s * yd.abs().sum(dim=(0, 2, 3)), 'c64 stats sum'))
    yd.mul_(yd)
    _report('c64 stats sumsq ' + tag, nr.check(part[:, 1].sum(0), yd.sum(dim=(0, 2, 3)), c_s * yd.sum(dim=(0, 2, 3)), 'c64 stats sumsq'))
    del yd, y, buf
    # inference: folded shift + residual + ReLU before the single rounding
    shift = torch.randn(64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed + 3))
    res = _act(n, 64, h, w, seed + 4, offset=False)
    buf, yb = _c64_call(x, wt, shift=shift, res=res, relu=1)
    _intact(buf, yb, 'c64 bias_act ' + tag)
    _stream_check('c64 shift+res+relu ' + tag, yb, x, wt, c, shift=shift, residual=res, relu=True)
    del yb, buf
    # the data gradient: the same kernel on the flipped filter, alone and with the residual branch's gradient added (zero shift)
    wf = nr.flip_filter(wt).contiguous(memory_format=CL)
    buf, gx = _c64_call(gy, wf)
    _intact(buf, gx, 'c64 dgrad ' + tag)
    _stream_check('c64 dgrad ' + tag, gx, gy, wf, c)
    buf, gx = _c64_call(gy, wf, shift=torch.zeros(64, device=DEV), res=res, relu=0)
    _intact(buf, gx, 'c64 dgrad + residual ' + tag)
    _stream_check('c64 dgrad + residual ' + tag, gx, gy, wf, c, residual=res)
    del gx, buf, res
    ref, absum = nr.conv_wgrad_ref(x, gy)
    for det in (False, True):
        nn_ops.set_deterministic(det, DEV)
        try:
            buf, dw = _guarded_dw((64, 3, 3, 64))
            with torch.cuda.device(DEV):
                assert L.salsa_nn_conv3x3_c64_wrw(P(x), P(gy), P(dw), n, h, w, S()) == 0
            torch.cuda.synchronize()
        finally:
            nn_ops.set_deterministic(False, DEV)
        what = 'c64 dW %s det=%d' % (tag, det)
        _intact(buf, dw, what)
        _report(what, nr.check(dw.permute(0, 3, 1, 2), ref, nr.c64_wgrad_c(n, h, w) * absum + 1e-30, what))


C64_LITE = [(320, 95), (640, 191), (320, 47)]


@pytest.mark.parametrize('hw', C64_LITE, ids=['%dx%d' % hw for hw in C64_LITE])
def test_c64_conv_forward_and_gradients_at_the_lite_maps(hw):
    """salsa_nn_conv3x3_c64, _stats, _bias_act, the data gradient and _wrw at 320 x 95 (stage 1), 640 x 191 (the stem's second
    convolution) and 320 x 47 (n_fft 256), at the smallest batch with batch 32's plan and grids"""
    h, w = hw
    n = LITE_C64_BATCH[hw]
    L = _lib()
    tr = c64_config(L, n, h, w)[1]
    assert tr == c64_config(L, 32, h, w)[1] == (1 if hw == (320, 47) else 0)
    assert L.salsa_nn_conv3x3_c64_stats_blocks(n, h, w) == L.salsa_nn_conv3x3_c64_stats_blocks(32, h, w) == (1024 if hw == (640, 191) else 512)
    if not tr:
        assert w % 32 == 31                                            # every row ends in a 31-column partial tile
    _c64_case(n, h, w, 100 + w)


C64_EDGE = [(h, w) for h in (4, 5) for w in (31, 33, 47, 95, 191)]


@pytest.mark.parametrize('hw', C64_EDGE, ids=['%dx%d' % hw for hw in C64_EDGE])
def test_c64_conv_at_small_odd_width_maps(hw):
    """the same at N = 2 on maps of one or two tile rows (H = 4: whole tiles, 5: a one-row partial tile below) whose rows end in
    a 31-, 1-, 15- or 31-column partial tile; 4 x 31 is a single partial tile per image"""
    _c64_case(2, hw[0], hw[1], 200 + 7 * hw[0] + hw[1])


# --------------------------------------------------------------------------------------------- first layer
def _stem_call(x, wq, shift=None, relu=False, part=None):
    L = _lib()
    n, cin, h, w = x.shape
    buf, y = _guarded((n, 64, h, w))
    with torch.cuda.device(DEV):
        if part is not None:
            rc = L.salsa_nn_conv3x3_stem_stats(P(x), x.stride(0), x.stride(1), P(wq), P(y), P(part), n, cin, h, w, S())
        else:
            rc = L.salsa_nn_conv3x3_stem(P(x), x.stride(0), x.stride(1), P(wq), P(shift), P(y), int(relu), n, cin, h, w, S())
    assert rc == 0
    torch.cuda.synchronize()
    _intact(buf, y, 'stem %dx%dx%dx%d' % (n, cin, h, w))
    return y


@pytest.mark.parametrize('cropped', [False, True], ids=['whole', 'time-cropped view'])
def test_stem_forward_and_weight_gradient_at_the_lite_map(cropped):
    """salsa_nn_conv3x3_stem (plain, folded shift + ReLU), _stem_stats and _stem_wrw at N x 7 x 640 x 191 on feature-shaped
    input -- whole, and on the view x[:, :, :640] of the extractor's 641 frames (batch stride != Cin H W) -- against conv_fwd_ref /
    conv_wgrad_ref on the bf16-rounded operands, as test_stem_forward_and_weight_gradient_at_mel_map"""
    nn_ops = _ops()
    from test_baseline_training_gpu import _stem_wrw_c, _w_from_filter
    n, cin, h, w = LITE_STEM_BATCH, 7, 640, 191
    L = _lib()
    g = torch.Generator(device=DEV).manual_seed(300)
    wq = nn_ops._stem_filter(torch.randn((64, cin, 3, 3), device=DEV, generator=g) * 0.2)
    assert tuple(wq.shape) == (64, 10, 8) and nn_ops._stem_wrw_hip(cin)
    nb = L.salsa_nn_conv3x3_stem_stats_blocks(n, h, w)
    assert nb == 1024 == L.salsa_nn_conv3x3_stem_stats_blocks(32, h, w)
    x = _features(n, cin, h + 1, w, 301, 'features')[:, :, :h] if cropped else _features(n, cin, h, w, 301, 'features')
    assert (x.stride(0) != cin * h * w) == cropped and nn_ops._planar_rows(x) and nn_ops._c64_map_ok(n, h, w)
    xq = x.bfloat16().float()
    wf = _w_from_filter(wq, cin)
    c = nr.conv_accum_c(wq.shape[1] * wq.shape[2])
    tag = 'stem 7->64 %dx%dx%d%s' % (n, h, w, ' cropped view' if cropped else '')
    y = _stem_call(x, wq)
    _stream_check(tag + ' fwd', y, xq, wf, c)
    shift = torch.randn(64, device=DEV, generator=g) * 0.5
    ys = _stem_call(x, wq, shift, relu=True)
    _stream_check(tag + ' shift+relu', ys, xq, wf, c, shift=shift, relu=True)
    del ys
    part = torch.full((nb, 2, 64), float('nan'), dtype=torch.float64, device=DEV)
    yt = _stem_call(x, wq, part=part)
    assert torch.equal(yt, y)
    yd = y.double()
    torch.testing.assert_close(part.sum(0)[0], yd.sum(dim=(0, 2, 3)), rtol=1e-5, atol=1e-2)
    torch.testing.assert_close(part.sum(0)[1], (yd * yd).sum(dim=(0, 2, 3)), rtol=1e-5, atol=1e-2)
    del yd, yt, y
    gy = _act(n, 64, h, w, 302, offset=False)
    ref, absum = nr.conv_wgrad_ref(xq, gy)
    buf, dw = _guarded_dw((64, cin, 3, 3))
    with torch.cuda.device(DEV):
        assert L.salsa_nn_conv3x3_stem_wrw(P(x), x.stride(0), x.stride(1), P(gy), P(dw), n, cin, h, w, S()) == 0
    torch.cuda.synchronize()
    _intact(buf, dw, tag + ' dW')
    _report(tag + ' dW', nr.check(dw, ref, _stem_wrw_c(n, h, w) * absum + 1e-30, tag + ' dW'))


def test_stem_batchnorm_backward_modes_at_the_lite_map():
    """salsa_nn_conv3x3_stem_wrw_bnf and _wrw_bn (the first layer's weight gradient with its BatchNorm + ReLU backward folded in)
    at 640 x 191 on feature-shaped input: the assertions of test_stem_batchnorm_backward_modes_at_mel_map"""
    from test_nn_kernels_at_scale_gpu import test_stem_batchnorm_backward_modes_at_mel_map as modes
    modes(7, 'features', shape=(LITE_STEM_BATCH, 640, 191))


# --------------------------------------------------------------------------------------------- wide 3x3
def _wide_call(x, wt, shift=None, res=None, relu=0, part=None):
    L = _lib()
    n, cin, h, w = x.shape
    cout = wt.shape[0]
    buf, y = _guarded((n, cout, h, w))
    with torch.cuda.device(DEV):
        if part is not None:
            rc = L.salsa_nn_conv3x3_wide_stats(P(x), P(wt), P(y), P(part), n, h, w, cin, cout, S())
        elif shift is None:
            rc = L.salsa_nn_conv3x3_wide(P(x), P(wt), P(y), n, h, w, cin, cout, S())
        else:
            rc = L.salsa_nn_conv3x3_wide_bias_act(P(x), P(wt), P(shift), P(res), P(y), relu, n, h, w, cin, cout, S())
    assert rc == 0
    torch.cuda.synchronize()
    _intact(buf, y, 'wide %d->%d %dx%dx%d' % (cin, cout, n, h, w))
    return y


def _layer_id(layer):
    return '%d->%d@%dx%d' % layer


@pytest.mark.parametrize('layer', LITE_GPU_WIDE, ids=_layer_id)
def test_wide_conv_forward_stats_and_folded_epilogue_at_the_lite_maps(layer):
    """salsa_nn_conv3x3_wide, _wide_stats and _wide_bias_act at every LITE_WIDE layer and at the three layers only another family
    reaches -- 64 -> 128 at 160 x 95 (n_fft 1024: (256, 128), no 512-pixel tile fits), 128 -> 256 at 80 x 47, 256 -> 512 at 40 x 5
    (n_fft 256) -- with the bounds of test_wide_conv_forward_stats_and_folded_epilogue"""
    cin, cout, h, w = layer
    n = LITE_BATCH[layer]
    L = _lib()
    inst = config(L, n, h, w, cout)
    assert L.salsa_nn_conv3x3_wide_supported(n, h, w, cin, cout) and inst == config(L, 32, h, w, cout) == wide_tile(32, h, w, cout)
    if layer == LITE1024_WIDE[0]:
        assert inst == (256, 128)
    if layer == LITE256_WIDE[4]:
        assert inst == (256, 64)
    x, wt = _act(n, cin, h, w, 1), _filt(cout, cin, 3, 2)
    ref, absum = nr.conv_fwd_ref(x, wt)
    c = nr.conv_accum_c(9 * cin)
    tag = '%s %d->%d %dx%dx%d' % (inst, cin, cout, n, h, w)
    y = _wide_call(x, wt)
    _report('wide fwd ' + tag, nr.check(y, ref, nr.bf16_bound(ref, absum, c), 'wide fwd ' + tag))
    blocks = L.salsa_nn_conv3x3_wide_stats_blocks(n, h, w, cin, cout)
    assert blocks == (n * h * w + inst[0] - 1) // inst[0]
    part = torch.full((blocks, 2, cout), float('nan'), dtype=torch.float64, device=DEV)
    ys = _wide_call(x, wt, part=part)
    assert torch.equal(ys, y)
    yd = y.double()
    # a tile's sums: float32 over its 64 pixels per wave (a pair add, two DPP steps, three shuffles: depth 7), then float64
    s_b = 8 * nr.U32 * yd.abs().sum(dim=(0, 2, 3))
    q_b = 8 * nr.U32 * (yd * yd).sum(dim=(0, 2, 3))
    _report('wide stats sum ' + tag, nr.check(part[:, 0].sum(0), yd.sum(dim=(0, 2, 3)), s_b, 'stats sum ' + tag))
    _report('wide stats sumsq ' + tag, nr.check(part[:, 1].sum(0), (yd * yd).sum(dim=(0, 2, 3)), q_b, 'stats sumsq ' + tag))
    shift = torch.randn(cout, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    res = _act(n, cout, h, w, 4, offset=False)
    yb = _wide_call(x, wt, shift=shift, res=res, relu=1)
    refb = (ref + shift.double().view(1, -1, 1, 1) + res.double()).clamp_(min=0)
    absb = absum + shift.double().abs().view(1, -1, 1, 1) + res.double().abs()
    _report('wide shift+res+relu ' + tag, nr.check(yb, refb, nr.bf16_bound(refb, absb, c), 'wide bias_act ' + tag))


@pytest.mark.parametrize('layer', LITE_GPU_WIDE, ids=_layer_id)
def test_wide_conv_data_gradient_at_the_lite_maps(layer):
    """the data gradient (a Cout -> Cin convolution on the flipped filter) of the same layers; 128 -> 256 at 80 x 47 is the
    (512, 128) data gradient no 200- or 128-bin map reaches"""
    cin, cout, h, w = layer
    n = LITE_BATCH[layer]
    L = _lib()
    inst = config(L, n, h, w, cin)
    assert L.salsa_nn_conv3x3_wide_supported(n, h, w, cout, cin) and inst == config(L, 32, h, w, cin) == wide_tile(32, h, w, cin)
    if layer == LITE1024_WIDE[2]:
        assert inst == (512, 128)
    gy, wt = _act(n, cout, h, w, 5), _filt(cout, cin, 3, 6)
    wf = nr.flip_filter(wt).contiguous(memory_format=CL)
    gx = _wide_call(gy, wf)
    ref, absum = nr.conv_fwd_ref(gy, wf)
    tag = '%s dgrad of %d->%d %dx%dx%d' % (inst, cin, cout, n, h, w)
    _report('wide ' + tag, nr.check(gx, ref, nr.bf16_bound(ref, absum, nr.conv_accum_c(9 * cout)), tag))


@pytest.mark.parametrize('layer', [l for l in LITE_GPU_WIDE if wide_wrw_ok(l[2], l[3])], ids=_layer_id)
def test_wide_conv_weight_gradient_at_the_lite_maps(layer):
    """salsa_nn_conv3x3_wide_wrw where the library takes the map: the generic (W2C = 0) kernel on three tile buffers, atomic and
    deterministic, within wide_wgrad_c's chain"""
    nn_ops = _ops()
    cin, cout, h, w = layer
    n = LITE_BATCH[layer]
    L = _lib()
    assert L.salsa_nn_conv3x3_wide_wrw_supported(n, h, w, cin, cout) and L.salsa_nn_conv3x3_wide_wrw_supported(32, h, w, cin, cout)
    assert wrw3(h, w) and w not in WRW_IMMEDIATE_W
    x, gy = _act(n, cin, h, w, 7), _act(n, cout, h, w, 8, offset=False)
    ref, absum = nr.conv_wgrad_ref(x, gy)
    vpos, inv, tb = nn_ops._wide_tables(n, h, w, DEV)
    for det in (False, True):
        nn_ops.set_deterministic(det, DEV)
        try:
            buf, dw = _guarded_dw((cout, 3, 3, cin))
            with torch.cuda.device(DEV):
                assert L.salsa_nn_conv3x3_wide_wrw(P(x), P(gy), P(dw), P(vpos), P(inv), P(tb), n, h, w, cin, cout, S()) == 0
            torch.cuda.synchronize()
        finally:
            nn_ops.set_deterministic(False, DEV)
        tag = 'wide dW 3 buffers generic W=%d %d->%d %dx%dx%d det=%d' % (w, cin, cout, n, h, w, det)
        _intact(buf, dw, tag)
        _report(tag, nr.check(dw.permute(0, 3, 1, 2), ref, nr.wide_wgrad_c(n, h, w, cin, cout) * absum, tag))


def test_wide_weight_gradient_at_160x95_is_refused_and_torch_takes_it():
    """64 -> 128 at 160 x 95 (n_fft 1024, stage 2): a 128-pixel tile's seven input rows of 97 slots need 43 456 B, the weight
    gradient's tile buffer holds 28 672 B, so salsa_nn_conv3x3_wide_wrw_supported answers 0, the entry point returns -1 without
    touching dW, and _Conv3x3Wide.backward takes that one gradient from torch (the data gradient stays on conv_wide.hip).  The
    fallback's bf16 dW against float64: float32 accumulation in an order this test does not know (any_order_wgrad_bound)."""
    nn_ops = _ops()
    cin, cout, h, w = LITE1024_WIDE[0]
    n = LITE_BATCH[LITE1024_WIDE[0]]
    L = _lib()
    assert not wide_wrw_ok(h, w) and not wrw3(h, w)
    for k in (n, 32):
        assert not L.salsa_nn_conv3x3_wide_wrw_supported(k, h, w, cin, cout) and L.salsa_nn_conv3x3_wide_supported(k, h, w, cout, cin)
    x, gy = _act(n, cin, h, w, 7), _act(n, cout, h, w, 8, offset=False)
    vpos, inv, tb = nn_ops._wide_tables(n, h, w, DEV)
    buf, dw = _guarded_dw((cout, 3, 3, cin))
    with torch.cuda.device(DEV):
        assert L.salsa_nn_conv3x3_wide_wrw(P(x), P(gy), P(dw), P(vpos), P(inv), P(tb), n, h, w, cin, cout, S()) == -1
    torch.cuda.synchronize()
    _intact(buf, dw, 'refused wide dW')
    assert not bool(dw.any())
    wt = torch.nn.Parameter(_filt(cout, cin, 3, 9).float())
    xa = x.clone().requires_grad_(True)
    y = nn_ops._Conv3x3Wide.apply(xa, wt)
    y.backward(gy)
    ref, absum = nr.conv_wgrad_ref(x, gy)
    tag = 'wide dW torch fallback %d->%d %dx%dx%d' % (cin, cout, n, h, w)
    assert wt.grad.dtype == torch.float32 and wt.grad.shape == (cout, cin, 3, 3)
    _report(tag, nr.check(wt.grad, ref, nr.any_order_wgrad_bound(ref, absum, n * h * w), tag))
    wf = nr.flip_filter(wt.detach().to(torch.bfloat16)).contiguous(memory_format=CL)
    ref, absum = nr.conv_fwd_ref(gy, wf)
    tag = '%s dgrad beside the fallback' % (config(L, n, h, w, cin),)
    _report('wide ' + tag, nr.check(xa.grad, ref, nr.bf16_bound(ref, absum, nr.conv_accum_c(9 * cout)), tag))


# --------------------------------------------------------------------------------------------- 1x1 shortcuts
@pytest.mark.parametrize('sc', [LITE_WIDE[0], LITE_WIDE[2], LITE_WIDE[4]], ids=_layer_id)
def test_conv1x1_both_instantiations_and_weight_gradient_at_the_lite_maps(sc):
    """salsa_nn_conv1x1 (<4> for Cout % 128 == 0, <2> for the 64-channel data gradient) and _wrw at the three stride-2 blocks'
    maps, N = 2: M = 15 040 (235 whole 64-pixel tiles), 3 680 and 880 rows (a last tile of 32 / 48 pixels)"""
    cin, cout, h, w = sc
    n = 2
    M = n * h * w
    assert M % 64 == {47: 0, 23: 32, 11: 48}[w]
    L = _lib()
    x, gy, wt = _act(n, cin, h, w, 12), _act(n, cout, h, w, 13, offset=False), _filt(cout, cin, 1, 14)
    for name, a, f in (('fwd', x, wt), ('dgrad', gy, wt.transpose(0, 1).contiguous())):
        assert L.salsa_nn_conv1x1_supported(M, f.shape[1], f.shape[0])
        nt = 4 if f.shape[0] % 128 == 0 else 2
        buf, y = _guarded((n, f.shape[0], h, w))
        with torch.cuda.device(DEV):
            assert L.salsa_nn_conv1x1(P(a), P(f), P(y), M, f.shape[1], f.shape[0], S()) == 0
        torch.cuda.synchronize()
        tag = '1x1 %s <%d> %d->%d M=%d' % (name, nt, f.shape[1], f.shape[0], M)
        _intact(buf, y, tag)
        ref, absum = nr.conv_fwd_ref(a, f)
        _report(tag, nr.check(y, ref, nr.bf16_bound(ref, absum, nr.conv_accum_c(f.shape[1])), tag))
    assert L.salsa_nn_conv1x1_wrw_supported(M, cin, cout)
    buf, dw = _guarded_dw((cout, cin))
    with torch.cuda.device(DEV):
        assert L.salsa_nn_conv1x1_wrw(P(x), P(gy), P(dw), M, cin, cout, S()) == 0
    torch.cuda.synchronize()
    tag = '1x1 dW %d->%d M=%d' % (cin, cout, M)
    _intact(buf, dw, tag)
    ref, absum = nr.conv_wgrad_ref(x, gy, k=1)
    _report(tag, nr.check(dw.view(cout, cin, 1, 1), ref, nr.conv1x1_wgrad_c(M, cin, cout) * absum, tag))


# --------------------------------------------------------------------------------------------- BatchNorm
def _bn_tensors(c, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.rand(c, device=DEV, generator=g) + 0.5, torch.randn(c, device=DEV, generator=g),
            torch.randn(c, device=DEV, generator=g), torch.rand(c, device=DEV, generator=g) + 0.5)


def _bn_train_direct(x, res, gy_of, pool, bits, gamma, beta, rm, rv, eps=1e-5, mom=0.1):
    """salsa_nn_bn_train_fwd[_pool][_bits] and salsa_nn_bn_bwd[_pool][_bits] as nn_ops._BnAct / _BnReluPool call them (ReLU on, no
    dropout), every output in a guarded NaN-filled buffer; gy_of(y shape) -> the upstream gradient.  -> y, gy, dx, dres, dgamma, dbeta"""
    nn_ops = _ops()
    L = _lib()
    n, c, h, w = x.shape
    M = n * h * w
    dt, lanes = nn_ops._DT[x.dtype]
    by, y = _guarded((n, c, h // 2, w // 2) if pool else (n, c, h, w), x.dtype)
    save = torch.full((2, c), float('nan'), device=DEV)
    ws = torch.empty(L.salsa_nn_bn_workspace_bytes(dt, M, c) // 8 + 1, dtype=torch.float64, device=DEV)
    plane = torch.full((x.numel() // lanes,), 0xA5, dtype=torch.uint8, device=DEV) if bits else None
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    head = (P(x), P(y), P(res), dt) + ((n, h, w, c) if pool else (M, c))
    mid = (P(gamma), P(beta), float(eps), float(mom), P(rm), P(rv), P(save[0]), P(save[1]), P(ws))
    tail = (P(count), None, 0) if pool else (1, 0.0, 0, P(count), None, 0)
    name = 'salsa_nn_bn_train_fwd' + ('_pool' if pool else '') + ('_bits' if bits else '')
    with torch.cuda.device(DEV):
        rc = getattr(L, name)(*(head + mid + tail + ((P(plane),) if bits else ()) + (S(),)))
    assert rc == 0, name
    torch.cuda.synchronize()
    _intact(by, y, name + ' y')
    assert int(count) == 1 and not bool(torch.isnan(save).any())
    gy = gy_of(y.shape)
    bdx, dx = _guarded((n, c, h, w), x.dtype)
    bdr, dres = _guarded((n, c, h, w), x.dtype) if res is not None else (None, None)
    dwb = torch.full((2, c), float('nan'), device=DEV)
    coef = torch.empty(7 * c, device=DEV)
    with torch.cuda.device(DEV):
        if pool:
            bname = 'salsa_nn_bn_bwd_pool' + ('_bits' if bits else '')
            rc = getattr(L, bname)(P(gy), P(x), P(plane if bits else res), P(dx), P(dres), dt, n, h, w, c, P(gamma), P(beta), P(save[0]),
                                   P(save[1]), P(dwb[0]), P(dwb[1]), P(ws), P(coef), S())
        else:
            bname = 'salsa_nn_bn_bwd'
            mask = plane if bits else (y if res is not None else None)      # (no residual: the mask is recomputed from x)
            rc = L.salsa_nn_bn_bwd(P(gy), P(mask), P(x), P(dx), P(dres), dt, M, c, P(gamma), P(beta), P(save[0]), P(save[1]),
                                   2 if bits else 1, P(dwb[0]), P(dwb[1]), P(ws), P(coef), 0.0, 0, S())
    assert rc == 0, bname
    torch.cuda.synchronize()
    _intact(bdx, dx, bname + ' dx')
    if res is not None:
        _intact(bdr, dres, bname + ' dres')
    assert not bool(torch.isnan(dwb).any())
    return y, gy, dx, dres, dwb[0], dwb[1]


def _bn_train_case(n, c, h, w, dtype, pool, variant):
    """variant: 'plain' (no residual: the mask recomputed from x), 'residual' (mask from the stored y, or from x and the residual
    under the pool) or 'bits' (residual, mask from the bit plane) -- against bn_train_ref / bn_bwd_ref with the bounds of
    test_batchnorm_train_forward_backward_at_bench_size"""
    bf16 = dtype == torch.bfloat16
    assert _lib().salsa_nn_bn_supported(1 if bf16 else 0, n * h * w, c)
    x = _act(n, c, h, w, 15).to(dtype)
    res = _act(n, c, h, w, 16, offset=False).to(dtype) if variant != 'plain' else None
    gamma, beta, rm, rv = _bn_tensors(c, 17)
    rm0, rv0 = rm.double().clone(), rv.double().clone()
    eps, m = 1e-5, 0.1
    y, gy, dx, dres, dgamma, dbeta = _bn_train_direct(x, res, lambda s: _act(s[0], c, s[2], s[3], 18, offset=False).to(dtype), pool,
                                                       variant == 'bits', gamma, beta, rm, rv, eps, m)
    r = nr.bn_train_ref(x, gamma, beta, eps, residual=res, relu=True, pool=pool)
    fwd_c = 16 * nr.U32
    tag = 'bn %s %s %s %dx%dx%dx%d' % ('pool' if pool else 'full', variant, 'bf16' if bf16 else 'fp32', n, c, h, w)
    yb = fwd_c * (F.avg_pool2d(r['fwd_abs'], 2) if pool else r['fwd_abs']) + (nr.BF16_REL * r['y'].abs() if bf16 else 0)
    _report(tag + ' y', nr.check(y, r['y'], yb, tag + ' y'))
    rm_ref = (1 - m) * rm0 + m * r['mean']
    rv_ref = (1 - m) * rv0 + m * r['unbiased']
    _report(tag + ' running_mean', nr.check(rm, rm_ref, 8 * nr.U32 * ((1 - m) * rm0.abs() + m * r['mean'].abs()), tag))
    rv_b = 8 * nr.U32 * ((1 - m) * rv0.abs() + m * r['unbiased'] * (1 + r['mean'] ** 2 / r['var']))
    _report(tag + ' running_var', nr.check(rv, rv_ref, rv_b, tag))
    b = nr.bn_bwd_ref(r, gamma, gy, relu=True, pool=pool, fwd_c=fwd_c, bf16=bf16)
    keep = ~b['exempt']
    _report(tag + ' dx', nr.check(dx.double()[keep], b['dx'][keep], b['b_dx'][keep], tag + ' dx'))
    if res is not None:
        _report(tag + ' dres', nr.check(dres.double()[keep], b['dres'][keep], b['b_dres'][keep], tag + ' dres'))
        if pool:
            # the gradient that passes straight through to the residual is +0.0 in the column (and row) the pool drops; dx there
            # is -a (dbeta + xhat dgamma) / M, not zero, and is held to bn_bwd_ref like every other element
            nr.assert_dropped_plus_zero(dres, tag + ' dres')
    _report(tag + ' dgamma', nr.check(dgamma, b['dgamma'], b['b_dgamma'], tag + ' dgamma'))
    _report(tag + ' dbeta', nr.check(dbeta, b['dbeta'], b['b_dbeta'], tag + ' dbeta'))
    assert int(keep.sum()) >= keep.numel() * (1 - 1e-4)            # (few undecided ReLU masks)


BN_MAPS = LITE_STAGES + [(128, 159, 47)]                            # (the last: odd H as well -- the pool drops a row and a column)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('variant', ['plain', 'residual', 'bits'])
@pytest.mark.parametrize('pool', [False, True], ids=['full', 'pool'])
@pytest.mark.parametrize('stage', BN_MAPS, ids=lambda s: '%dx%dx%d' % s)
def test_batchnorm_train_forward_backward_at_the_lite_maps(stage, pool, variant, dtype):
    """salsa_nn_bn_train_fwd / _fwd_bits / _fwd_pool / _fwd_pool_bits and salsa_nn_bn_bwd / _bwd_pool / _bwd_pool_bits at every
    Lite stage (and 159 x 47), N = 2, both dtypes: every width is odd, so each pooled variant drops a column"""
    c, h, w = stage
    assert w % 2 == 1
    _bn_train_case(2, c, h, w, dtype, pool, variant)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('stage', BN_MAPS, ids=lambda s: '%dx%dx%d' % s)
def test_batchnorm_eval_forward_at_the_lite_maps(stage, dtype):
    """salsa_nn_bn_eval_fwd (residual + ReLU) on running statistics against bn_eval_ref: the training forward's 16 u of
    |gamma| invstd (|x| + |mean|) + |beta| + |residual| (+ one bf16 rounding); invstd is the float32 rsqrt(running_var + eps) that
    BatchNormAct2d.forward hands the kernel, an operand of the reference as well."""
    nn_ops = _ops()
    c, h, w = stage
    n = 2
    bf16 = dtype == torch.bfloat16
    dt = nn_ops._DT[dtype][0]
    assert _lib().salsa_nn_bn_supported(dt, n * h * w, c)
    x, res = _act(n, c, h, w, 19).to(dtype), _act(n, c, h, w, 20, offset=False).to(dtype)
    gamma, beta, rm, rv = _bn_tensors(c, 21)
    invstd = torch.rsqrt(rv + 1e-5)
    buf, y = _guarded((n, c, h, w), dtype)
    with torch.cuda.device(DEV):
        assert _lib().salsa_nn_bn_eval_fwd(P(x), P(y), P(res), dt, n * h * w, c, P(gamma), P(beta), P(rm), P(invstd), 1, S()) == 0
    torch.cuda.synchronize()
    tag = 'bn eval %s %dx%dx%dx%d' % ('bf16' if bf16 else 'fp32', n, c, h, w)
    _intact(buf, y, tag)
    ref, absum = nr.bn_eval_ref(x, gamma, beta, rm, invstd, residual=res, relu=True)
    _report(tag, nr.check(y, ref, 16 * nr.U32 * absum + (nr.BF16_REL * ref.abs() if bf16 else 0), tag))


# --------------------------------------------------------------------------------------------- average pool
# (C, H, W) down the chain: the stem's pool in eval mode, then the pool behind stages 1 - 3; and an odd H
POOL_CHAIN = [(64, 640, 191), (64, 320, 95), (128, 160, 47), (256, 80, 23), (128, 159, 47)]


@pytest.mark.parametrize('chw', POOL_CHAIN, ids=lambda s: '%dx%dx%d' % s)
def test_avgpool_forward_and_backward_at_the_lite_maps(chw):
    """salsa_nn_avgpool2x2_fwd (avgpool_bound) and _bwd at 640 x 191 -> 320 x 95 and down the chain, N = 2.  The backward is
    exact (a division by 4: avgpool_bwd_ref) and writes +0.0 into the column -- at 159 x 47 also the row -- the pool drops."""
    nn_ops = _ops()
    c, h, w = chw
    n = 2
    L = _lib()
    x = _act(n, c, h, w, 22)
    dt = nn_ops._DT[x.dtype][0]
    buf, y = _guarded((n, c, h // 2, w // 2))
    with torch.cuda.device(DEV):
        assert L.salsa_nn_avgpool2x2_fwd(P(x), P(y), dt, n, h, w, c, S()) == 0
    torch.cuda.synchronize()
    tag = 'avg pool %dx%dx%dx%d -> %dx%d' % (n, c, h, w, h // 2, w // 2)
    _intact(buf, y, tag)
    ref, bound = nr.avgpool_bound(x)
    assert ref.shape == y.shape
    _report(tag, nr.check(y, ref, bound, tag))
    gy = _act(n, c, h // 2, w // 2, 23, offset=False)
    buf, gx = _guarded((n, c, h, w))
    with torch.cuda.device(DEV):
        assert L.salsa_nn_avgpool2x2_bwd(P(gy), P(gx), dt, n, h, w, c, S()) == 0
    torch.cuda.synchronize()
    _intact(buf, gx, tag + ' bwd')
    want = nr.avgpool_bwd_ref(gy, h, w)
    _report(tag + ' bwd (exact)', nr.check(gx, want, 0 * want, tag + ' bwd'))
    nr.assert_dropped_plus_zero(gx, tag + ' bwd')


# --------------------------------------------------------------------------------------------- frequency mean and pools
FREQ_MAPS = [(32, 512, 40, 11), (32, 512, 300, 11), (32, 512, 40, 23), (32, 512, 40, 5)]     # (300 rows: 60-s inference)


@pytest.mark.parametrize('shape', FREQ_MAPS, ids=lambda s: '%dx%dx%dx%d' % s)
def test_frequency_mean_at_the_lite_widths(shape):
    """salsa_nn_freq_mean_fwd / _bwd over 11, 23 and 5 bins: the assertions of test_frequency_mean_forward_and_backward_at_bench_size"""
    from test_nn_kernels_at_scale_gpu import test_frequency_mean_forward_and_backward_at_bench_size as case
    case(shape)


@pytest.mark.parametrize('mode', ['max', 'avg_max'])
@pytest.mark.parametrize('shape', FREQ_MAPS, ids=lambda s: '%dx%dx%dx%d' % s)
def test_frequency_pools_at_the_lite_widths(shape, mode):
    """salsa_nn_freq_pool_fwd / _bwd over 11, 23 and 5 bins on plain and tie-laden input, guarded buffers: the assertions of
    test_freq_pool_kernels_at_bench_size -- the argmax is the LOWEST index holding the maximum, everywhere"""
    from test_rnn_scans_at_scale_gpu import test_freq_pool_kernels_at_bench_size as case
    case(shape, mode)


# --------------------------------------------------------------------------------------------- the eval path of a 60-s clip
def test_eval_stem_conv2_with_the_unfused_pool_at_60_s():
    """conv_bn_act(pool=True) in eval mode at N x 64 x 4800 x 191: W is odd, so _conv_bn_act's fuse_pool is false and the stem runs
    salsa_nn_conv3x3_c64_bias_act -> salsa_nn_avgpool2x2_fwd (at 200 and 128 bins: one fused kernel).  The convolution against the
    streamed float64 reference; the pooled result is bit for bit the stand-alone pool of that output and within avgpool_bound of
    pool(output) -- together: pool(reference) within the mean of four bf16_bounds plus the pool's own bound."""
    nn_ops = _ops()
    from test_nn_kernels_full_res_gpu import _eval, _eval_pair
    h, w = 4800, 191
    n = LITE_C64_BATCH[(h, w)]
    L = _lib()
    tiles, tr = c64_config(L, n, h, w)
    assert (tiles, tr) == c64_plan(n, h, w) and tr == 0 and tiles >= 16384 and L.salsa_nn_conv3x3_c64_stats_blocks(n, h, w) == 1024
    assert not (h % 2 == 0 and w % 2 == 0)                               # fuse_pool = pool and H % 2 == 0 and W % 2 == 0: false
    conv, bn = _eval_pair(64, 64, 40)
    x = _act(n, 64, h, w, 41)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        assert conv._hip_eligible(x)
    full = _eval(conv, bn, x, relu=True, pool=False)
    pooled = _eval(conv, bn, x, relu=True, pool=True)
    assert full.shape == (n, 64, h, w) and pooled.shape == (n, 64, h // 2, w // 2) and pooled.dtype == torch.bfloat16
    assert pooled.is_contiguous(memory_format=CL)
    wf, shift = nn_ops._folded(conv, bn)
    tag = 'c64 eval <plain> %dx%dx%d untransposed (%d tiles / 1024)' % (n, h, w, tiles)
    _stream_check(tag, full, x, wf, nr.conv_accum_c(9 * 64), shift=shift, relu=True)
    assert torch.equal(pooled, nn_ops.avg_pool2x2(full))
    ref, bound = nr.avgpool_bound(full)
    _report('unfused avg pool %dx64x%dx%d -> %dx%d' % (n, h, w, h // 2, w // 2), nr.check(pooled, ref, bound, 'unfused pool'))


@pytest.mark.parametrize('variant', ['relu', 'residual+relu', 'residual+relu+pool'])
def test_eval_stage1_at_60_s(variant):
    """salsa_nn_conv3x3_c64_bias_act at N x 64 x 2400 x 95 on the 1024-workgroup grid, untransposed: a block's first convolution,
    its second (<residual-early>) and stage 1's last, whose pool (95 -> 47) is again a launch of its own"""
    nn_ops = _ops()
    from test_nn_kernels_full_res_gpu import _eval, _eval_pair
    h, w = 2400, 95
    n = LITE_C64_BATCH[(h, w)]
    L = _lib()
    tiles, tr = c64_config(L, n, h, w)
    assert tr == 0 and tiles >= 16384 and L.salsa_nn_conv3x3_c64_stats_blocks(n, h, w) == 1024
    conv, bn = _eval_pair(64, 64, 50)
    x = _act(n, 64, h, w, 51)
    res = _act(n, 64, h, w, 52, offset=False) if 'residual' in variant else None
    full = _eval(conv, bn, x, residual=res, relu=True, pool=False)
    wf, shift = nn_ops._folded(conv, bn)
    tag = 'c64 eval <%s> %dx%dx%d untransposed (%d tiles / 1024)' % (variant, n, h, w, tiles)
    _stream_check(tag, full, x, wf, nr.conv_accum_c(9 * 64), shift=shift, residual=res, relu=True)
    if 'pool' in variant:
        assert w % 2 == 1
        pooled = _eval(conv, bn, x, residual=res, relu=True, pool=True)
        assert pooled.shape == (n, 64, h // 2, w // 2) and torch.equal(pooled, nn_ops.avg_pool2x2(full))
        ref, bound = nr.avgpool_bound(full)
        _report('unfused avg pool %dx64x%dx%d -> %dx%d' % (n, h, w, h // 2, w // 2), nr.check(pooled, ref, bound, 'unfused pool'))


# --------------------------------------------------------------------------------------------- the whole model
def test_whole_model_hip_layers_on_vs_off_at_191_bins():
    """one bf16 training step and one eval forward of the CRNN on synthetic_batch(8, n_freq=191), every hand-written layer on,
    against the torch-layer leg: the switches and bounds of test_whole_model_hip_layers_on_vs_off"""
    from salsa_amd.crnn.train import synthetic_batch
    from test_crnn_gpu import whole_model_hip_layers_on_vs_off
    x, sed, doa = synthetic_batch(8, DEV, seed=3, n_freq=191)
    assert x.shape == (8, 7, 640, 191)
    whole_model_hip_layers_on_vs_off((x, sed, doa))


def test_deterministic_mode_gives_bit_equal_weight_gradients_at_191_bins():
    from test_crnn_gpu import deterministic_mode_gives_bit_equal_weight_gradients
    deterministic_mode_gives_bit_equal_weight_gradients(n_freq=191)


@pytest.mark.parametrize('n_fft,n_freq,clips', [(512, 191, 8), (1024, 382, 2)])
def test_on_the_fly_lite_features_feed_the_model(n_fft, n_freq, clips):
    """raw 8-s MIC audio -> SALSA-Lite on device (n_fft 512: 191 bins, 1024: 382) -> Trainer.train_step and Trainer.infer, no host
    round trip (test_on_the_fly_features_feed_the_model); then the HIP-layers-on against torch-layers comparison on those
    unnormalised features (log-spectrograms of mean ~0 and std ~20 dB, NIPD channels within +-1).  8 clips at 191 bins: the torch
    legs then meet the maps MIOpen has already searched for the synthetic batch above; 382 bins stays at 2 clips."""
    from salsa_amd.crnn.train import Trainer, synthetic_batch
    from salsa_amd.extractor import SalsaExtractor
    from salsa_amd.synth import synth_clip
    from test_crnn_gpu import whole_model_hip_layers_on_vs_off
    ys = np.stack([synth_clip(60 + i, 8 * 24000) for i in range(clips)])
    feats = SalsaExtractor(audio_format='mic', feature_type='salsa_lite', n_fft=n_fft, fmax_doa=2000).extract(torch.from_numpy(ys).to(DEV))
    assert feats.shape == (clips, 7, 641, n_freq)
    tr = Trainer('cuda:0', total_steps=10)
    _, sed, doa = synthetic_batch(clips, 'cuda:0', seed=2)
    x = feats[:, :, :640]
    loss = tr.train_step(x, sed, doa)[0]
    assert np.isfinite(float(loss))
    p, d = tr.infer(x)
    assert p.shape == (clips, 80, 12) and d.shape == (clips, 80, 36)
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(d).all()) and float(p.min()) >= 0 and float(p.max()) <= 1
    # the DOA loss is a masked L1: one sign flip among the 84 active labels of an axis (2 clips) is 0.21 of that axis' loss gradient
    # (see the helper).  Labels within 5e-2 -- the tolerance the helper itself grants two legs' outputs -- of their float32
    # prediction are switched off first
    whole_model_hip_layers_on_vs_off((x, sed, doa), label_margin=5e-2)
