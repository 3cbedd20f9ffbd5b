"""The CRNN's hand-written kernels at the two families of maps tests/test_nn_kernels_at_scale_gpu.py does not reach -- the
largest launches of the project: the stem's second convolution in training (32 x 64 x 640 x {200, 128}) and the whole eval
path of a batch of 32 clips of 60 s (Trainer.infer on 32 x (7, 4800, 200)).  Same conventions as the at-scale file: inputs
from _act / _filt, every case first asserts the instantiation / grid it reaches, _report prints max err / bound, bounds are
the per-element ones of tests/nn_reference.py, every output element of every clip is checked.  The float64 reference of a
4800- or 2400-row map is streamed band by band (nr.conv_fwd_ref_stream): the whole-batch float64 tensor never exists, and
every test prints its peak device memory.  Run alone:
python -m pytest -m gpu tests/test_nn_kernels_full_res_gpu.py -q -s

  launch                                     tiles, geometry         what only this file reaches
  c64 32 x 640 x 200 (training stem conv2)   32 000, transposed      the 1024-workgroup persistent grid (>= 16384 tiles), ~31 tiles each
  c64 32 x 640 x 128 (mel)                   20 480, untransposed    1024 grid, untransposed
  c64 weight gradient 32 x 640 x {200, 128}  32 000 / 20 480         its 512-workgroup grid, 63 / 40 tiles each
  BatchNorm + ReLU + pool, M = 4 096 000     -                       rows beyond 1 024 000, fed by the 1024-row partial table
  c64 32 x 4800 x 200 (inference stem conv2) 240 000, transposed     ~234 tiles per workgroup, pool + transposed output strides, 3.93 GB
  c64 32 x 4800 x 128 / 2400 x 64 (mel)      153 600 / 38 400        1024 grid, untransposed, pool
  c64 32 x 2400 x 100 (inference stage 1)    60 000, transposed      <residual-early> and <pool, residual-early> on the 1024 grid
  stem 32 x 7 x 4800 x 200, 10 x 4800 x 128  -                       a time-cropped view (batch stride != Cin H W), folded shift + ReLU
  wide 32 x 1200 x 50 / 600 x 25 (x 32 / 16) (512, 128)              7.5 x the tiles of training; residual + folded shortcut shift
  wide 32 x 300 x 12 (x 8), Cout 512         (512, 128)              the 512-pixel tile at W = 12 / 8 (training: (256, 128) / (256, 64))
  average pool 1200 x 50, 600 x 25           -                       an odd width (25 -> 12)
  c64_xform_stats, c64_wrw_xform, bn_train_finalize                  no caller in the package: tested here only

Wall time on one MI355X: 13 s for the 30 cases (profiles/nn_full_res_pytest_gpu.log); peak device memory 34 GB (the float32
BatchNorm case at M = 4 096 000, whose float64 reference is held whole), 16 GB for the 3.93-GB convolution.
"""
import pytest
import torch

import nn_reference as nr
from test_nn_kernels_at_scale_gpu import CL, DEV, _act, _features, _filt, _lib, _report
from test_nn_reference_cpu import C64_FULL_RES, WIDE_FULL_RES, c64_config, c64_plan, config, wide_tile

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _peak_memory(request):
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    print('%-58s peak memory %.2f GB' % (request.node.name[:58], torch.cuda.max_memory_allocated() / 1e9))
    torch.cuda.empty_cache()


def _geo(n, h, w):
    """asserts the 64 -> 64 plan of a full-resolution map (tiles, transposed) and its 1024-workgroup grid; -> (tiles, transposed)"""
    L = _lib()
    geo = dict(C64_FULL_RES)[(n, h, w)]
    assert c64_config(L, n, h, w) == geo == c64_plan(n, h, w) and geo[0] >= 16384
    assert L.salsa_nn_conv3x3_c64_stats_blocks(n, h, w) == 1024          # (the grid every c64 forward entry point picks by this rule)
    return geo


def _stream_check(what, y, x, w, c, **kw):
    """y against the streamed float64 reference, every piece of every clip; reports and returns the maximum err / bound"""
    worst, rows = 0.0, 0
    for (n, a, b), ref, absum in nr.conv_fwd_ref_stream(x, w, **kw):
        worst = max(worst, nr.check(y[n:n + 1, :, a:b], ref, nr.bf16_bound(ref, absum, c), '%s, clip %d rows %d:%d' % (what, n, a, b)))
        rows += b - a
        del ref, absum
    assert rows == y.shape[0] * y.shape[2]
    return _report(what, worst)


def _eval_pair(cin, cout, seed):
    """a Conv3x3 + BatchNormAct2d pair in eval mode with non-trivial running statistics"""
    from salsa_amd.crnn import nn_ops
    g = torch.Generator(device=DEV).manual_seed(seed)
    conv = nn_ops.Conv3x3(cin, cout, 3, padding=1, bias=False).to(DEV).eval()
    bn = nn_ops.BatchNormAct2d(cout).to(DEV).eval()
    with torch.no_grad():
        conv.weight.copy_(torch.randn((cout, cin, 3, 3), device=DEV, generator=g) * (2.0 / (9 * cin)) ** 0.5)
        bn.weight.copy_(torch.rand(cout, device=DEV, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(cout, device=DEV, generator=g))
        bn.running_mean.copy_(torch.randn(cout, device=DEV, generator=g) * 0.5)
        bn.running_var.copy_(torch.rand(cout, device=DEV, generator=g) + 0.5)
    return conv, bn


def _eval(conv, bn, x, **kw):
    from salsa_amd.crnn import nn_ops
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
        return nn_ops.conv_bn_act(conv, bn, x, **kw)


# --------------------------------------------------------------------------------------------- training, stem conv2
STEM2 = [(640, 200), (640, 128)]


@pytest.mark.parametrize('hw', STEM2, ids=['%dx%d' % hw for hw in STEM2])
def test_c64_conv_forward_and_gradients_at_the_stem_map(hw):
    """salsa_nn_conv3x3_c64, _stats, the data gradient and _wrw at 32 x 64 x 640 x {200, 128}: four times the pixels of the
    residual stage, the 1024-workgroup grid (31 / 20 tiles per workgroup).  The statistics chain in float32: a row pair (1), two
    DPP steps (2), the lane's running sum over ceil(tiles / 1024) tiles, three shuffles (3), + 2 spare: (ceil(tiles / blocks) + 8) u."""
    from salsa_amd.crnn import nn_ops
    n, (h, w) = 32, hw
    L = _lib()
    tiles, tr = _geo(n, h, w)
    blocks = L.salsa_nn_conv3x3_c64_stats_blocks(n, h, w)
    tag = '%dx%dx%d %s' % (n, h, w, 'transposed' if tr else 'untransposed')
    x, gy, wt = _act(n, 64, h, w, 31), _act(n, 64, h, w, 32, offset=False), _filt(64, 64, 3, 33)
    c = nr.conv_accum_c(9 * 64)
    y = nn_ops._conv64(x, wt)
    _stream_check('c64 fwd ' + tag, y, x, wt, c)
    part = torch.full((blocks, 2, 64), float('nan'), dtype=torch.float64, device=DEV)
    ys = nn_ops._conv64(x, wt, stats_part=part)
    assert torch.equal(ys, y)
    del ys
    yd = y.double()
    c_s = (-(-tiles // blocks) + 8) * nr.U32
    _report('c64 stats sum ' + tag, nr.check(part[:, 0].sum(0), yd.sum(dim=(0, 2, 3)), c_s * yd.abs().sum(dim=(0, 2, 3)), 'c64 stats sum'))
    yd.mul_(yd)
    _report('c64 stats sumsq ' + tag, nr.check(part[:, 1].sum(0), yd.sum(dim=(0, 2, 3)), c_s * yd.sum(dim=(0, 2, 3)), 'c64 stats sumsq'))
    del yd, y
    wf = nr.flip_filter(wt).contiguous(memory_format=CL)
    gx = nn_ops._conv64(gy, wf)
    _stream_check('c64 dgrad ' + tag, gx, gy, wf, c)
    del gx
    ref, absum = nr.conv_wgrad_ref(x, gy)
    for det in (False, True):
        nn_ops.set_deterministic(det, DEV)
        try:
            dw = torch.zeros((64, 3, 3, 64), dtype=torch.float32, device=DEV)
            with torch.cuda.device(DEV):
                assert L.salsa_nn_conv3x3_c64_wrw(nn_ops._ptr(x), nn_ops._ptr(gy), nn_ops._ptr(dw), n, h, w, nn_ops._stream(x)) == 0
            torch.cuda.synchronize()
        finally:
            nn_ops.set_deterministic(False, DEV)
        what = 'c64 dW %s det=%d' % (tag, det)
        _report(what, nr.check(dw.permute(0, 3, 1, 2), ref, nr.c64_wgrad_c(n, h, w) * absum, what))


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'fp32'])
@pytest.mark.parametrize('hw', STEM2, ids=['%dx%d' % hw for hw in STEM2])
def test_batchnorm_relu_pool_at_the_stem_map_fed_by_the_conv_statistics(hw, dtype):
    """BatchNormAct2d.relu_pool forward and backward at M = 4 096 000 rows (C = 64), its batch statistics taken from the
    1024-row partial table salsa_nn_conv3x3_c64_stats left (the training path of the stem), against bn_train_ref / bn_bwd_ref
    with the bounds of test_batchnorm_train_forward_backward_at_bench_size (fwd_c = 16 u, at most 1e-4 undecided ReLU masks).
    float32: the same values (the bf16 output cast up exactly), so the same partial table describes them."""
    from salsa_amd.crnn import nn_ops
    n, (h, w), c = 32, hw, 64
    bf16 = dtype == torch.bfloat16
    L = _lib()
    tiles, _ = _geo(n, h, w)
    assert L.salsa_nn_bn_supported(1 if bf16 else 0, n * h * w, c)
    part = torch.full((1024, 2, 64), float('nan'), dtype=torch.float64, device=DEV)
    x = nn_ops._conv64(_act(n, 64, h, w, 34), _filt(64, 64, 3, 35), stats_part=part).to(dtype)
    bn = nn_ops.BatchNormAct2d(c).to(DEV).train()
    g = torch.Generator(device=DEV).manual_seed(36)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, device=DEV, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(c, device=DEV, generator=g))
        bn.running_mean.copy_(torch.randn(c, device=DEV, generator=g))
        bn.running_var.copy_(torch.rand(c, device=DEV, generator=g) + 0.5)
    rm0, rv0 = bn.running_mean.double().clone(), bn.running_var.double().clone()
    xa = x.clone().requires_grad_(True)
    y = bn.relu_pool(xa, part.view(-1))
    assert isinstance(y.grad_fn, nn_ops._BnReluPool._backward_cls)
    gy = _act(n, c, h // 2, w // 2, 37, offset=False).to(dtype)
    y.backward(gy)
    r = nr.bn_train_ref(x, bn.weight.detach(), bn.bias.detach(), bn.eps, relu=True, pool=True)
    fwd_c = 16 * nr.U32
    tag = 'bn pool %s C=%d M=%d from conv stats' % ('bf16' if bf16 else 'fp32', c, r['M'])
    yb = fwd_c * torch.nn.functional.avg_pool2d(r['fwd_abs'], 2) + (nr.BF16_REL * r['y'].abs() if bf16 else 0)
    _report(tag + ' y', nr.check(y.detach(), r['y'], yb, tag + ' y'))
    del yb
    # the statistics' own chain (the convolution's float32 partial sums, test above) on top of the BatchNorm's constants
    c_s = (-(-tiles // 1024) + 8) * nr.U32
    xd_abs = x.double().abs().mean(dim=(0, 2, 3))
    m = bn.momentum
    rm_ref = (1 - m) * rm0 + m * r['mean']
    rv_ref = (1 - m) * rv0 + m * r['unbiased']
    rm_b = 8 * nr.U32 * ((1 - m) * rm0.abs() + m * r['mean'].abs()) + m * c_s * xd_abs
    _report(tag + ' running_mean', nr.check(bn.running_mean, rm_ref, rm_b, tag))
    rv_b = 8 * nr.U32 * ((1 - m) * rv0.abs() + m * r['unbiased'] * (1 + r['mean'] ** 2 / r['var'])) \
        + m * c_s * ((r['var'] + r['mean'] ** 2) + 2 * r['mean'].abs() * xd_abs)
    _report(tag + ' running_var', nr.check(bn.running_var, rv_ref, rv_b, tag))
    b = nr.bn_bwd_ref(r, bn.weight.detach(), gy, relu=True, pool=True, fwd_c=fwd_c, bf16=bf16)
    keep = ~b['exempt']
    _report(tag + ' dx', nr.check(xa.grad.double()[keep], b['dx'][keep], b['b_dx'][keep], tag + ' dx'))
    _report(tag + ' dgamma', nr.check(bn.weight.grad, b['dgamma'], b['b_dgamma'], tag + ' dgamma'))
    _report(tag + ' dbeta', nr.check(bn.bias.grad, b['dbeta'], b['b_dbeta'], tag + ' dbeta'))
    assert int(keep.sum()) >= keep.numel() * (1 - 1e-4)            # (few undecided ReLU masks)


# --------------------------------------------------------------------------------------------- inference, 64 -> 64
def _c64_eval_case(n, h, w, residual, pool, seed):
    """conv_bn_act in eval mode under bf16 autocast at one full-resolution map, against the streamed float64 reference on the
    folded bf16 filter and float32 shift of nn_ops._folded"""
    from salsa_amd.crnn import nn_ops
    tiles, tr = _geo(n, h, w)
    conv, bn = _eval_pair(64, 64, seed)
    x = _act(n, 64, h, w, seed + 1)
    res = _act(n, 64, h, w, seed + 2, offset=False) if residual else None
    with torch.autocast('cuda', dtype=torch.bfloat16):
        assert conv._hip_eligible(x) and h % 2 == 0 and w % 2 == 0     # -> salsa_nn_conv3x3_c64_bias_act[_pool], pool fused
    y = _eval(conv, bn, x, residual=res, relu=True, pool=pool)
    assert y.dtype == torch.bfloat16 and y.shape == ((n, 64, h // 2, w // 2) if pool else (n, 64, h, w))
    assert y.is_contiguous(memory_format=CL)
    wf, shift = nn_ops._folded(conv, bn)
    assert wf.dtype == torch.bfloat16 and shift.dtype == torch.float32
    inst = '<%s%s>' % ('pool' if pool else 'plain', ', residual-early' if residual else '')
    tag = 'c64 eval %s %dx%dx%d %s (%d tiles / 1024)' % (inst, n, h, w, 'transposed' if tr else 'untransposed', tiles)
    c = nr.pooled_conv_c(9 * 64) if pool else nr.conv_accum_c(9 * 64)
    return _stream_check(tag, y, x, wf, c, shift=shift, residual=res, relu=True, pool=pool)


@pytest.mark.parametrize('w', [200, 128])
def test_c64_eval_stem_conv2_with_fused_pool_at_60_s(w):
    """salsa_nn_conv3x3_c64_bias_act_pool at 32 x 4800 x {200, 128}: the largest launch of the project (input 3.93 GB at 200
    bins, element offsets up to 92 % of 2^31); the last clip's last band is the highest address any kernel here touches"""
    _c64_eval_case(32, 4800, w, residual=False, pool=True, seed=40)


@pytest.mark.parametrize('variant', ['relu', 'residual+relu', 'residual+relu+pool'])
@pytest.mark.parametrize('w', [100, 64])
def test_c64_eval_stage1_at_60_s(w, variant):
    """salsa_nn_conv3x3_c64_bias_act at 32 x 2400 x {100, 64}: a block's first convolution (ReLU), its second (residual + ReLU,
    the <residual-early> instantiation) and stage 1's last (residual + ReLU + pool: <pool, residual-early>)"""
    _c64_eval_case(32, 2400, w, residual='residual' in variant, pool='pool' in variant, seed=50)


# --------------------------------------------------------------------------------------------- inference, first layer
@pytest.mark.parametrize('cin,w', [(7, 200), (10, 128)])
def test_stem_eval_on_a_time_cropped_view_at_60_s(cin, w):
    """salsa_nn_conv3x3_stem with folded shift + ReLU at 32 x Cin x 4800 x W on the view x[:, :, :4800] of a (32, Cin, 4801, W)
    float32 tensor (batch stride != Cin H W, as Trainer.infer passes it); Cin = 10: the 16-channel layout.  Reference on the
    bf16-rounded input, as in test_stem_forward_and_weight_gradient_at_mel_map."""
    from salsa_amd.crnn import nn_ops
    from test_baseline_training_gpu import _w_from_filter
    n, h = 32, 4800
    g = torch.Generator(device=DEV).manual_seed(60 + cin)
    wq = nn_ops._stem_filter(torch.randn((64, cin, 3, 3), device=DEV, generator=g) * 0.2)
    assert tuple(wq.shape) == ((64, 10, 8) if cin <= 8 else (64, 9, 16))
    shift = torch.randn(64, device=DEV, generator=g) * 0.5
    x = _features(n, cin, h + 1, w, 61 + cin, 'features')[:, :, :h]
    assert x.stride(0) == cin * (h + 1) * w != cin * h * w and nn_ops._planar_rows(x) and nn_ops._c64_map_ok(n, h, w)
    y = nn_ops._conv_stem(x, wq, shift, relu=True)
    xq = x.bfloat16().float()
    _stream_check('stem eval %d->64 %dx%dx%d cropped view' % (cin, n, h, w), y, xq, _w_from_filter(wq, cin),
                  nr.conv_accum_c(wq.shape[1] * wq.shape[2]), shift=shift, relu=True)


# --------------------------------------------------------------------------------------------- inference, wide layers
# (Cin, Cout, H, W) of stages 2 - 4 at 32 clips of 60 s, 200-bin and 128-bin features
WIDE_EVAL = [(64, 128, 1200, 50), (128, 128, 1200, 50), (128, 256, 600, 25), (256, 256, 600, 25), (256, 512, 300, 12), (512, 512, 300, 12),
             (64, 128, 1200, 32), (128, 128, 1200, 32), (128, 256, 600, 16), (256, 256, 600, 16), (256, 512, 300, 8), (512, 512, 300, 8)]


@pytest.mark.parametrize('layer', WIDE_EVAL)
def test_wide_eval_layers_and_pools_at_60_s(layer):
    """salsa_nn_conv3x3_wide_bias_act through conv_bn_act (eval, bf16 autocast) at 32 clips: Cin != Cout is a block's first
    convolution (ReLU), Cin == Cout its second (residual + the folded shortcut's residual_shift + ReLU) followed, at the 1200-
    and 600-row maps, by salsa_nn_avgpool2x2_fwd of that output (600 x 25 -> 300 x 12: an odd width)."""
    from salsa_amd.crnn import nn_ops
    cin, cout, h, w = layer
    n = 32
    L = _lib()
    assert (n, h, w, cout) in WIDE_FULL_RES and L.salsa_nn_conv3x3_wide_supported(n, h, w, cin, cout)
    assert config(L, n, h, w, cout) == (512, 128) == wide_tile(n, h, w, cout)
    conv, bn = _eval_pair(cin, cout, 70)
    x = _act(n, cin, h, w, 71)
    second = cin == cout
    res = _act(n, cout, h, w, 72, offset=False) if second else None
    rs = torch.randn(cout, device=DEV, generator=torch.Generator(device=DEV).manual_seed(73)) if second else None
    with torch.autocast('cuda', dtype=torch.bfloat16):
        assert conv._wide_eligible(x) and not conv._hip_eligible(x)
    y = _eval(conv, bn, x, residual=res, relu=True, residual_shift=rs)
    assert y.dtype == torch.bfloat16 and y.shape == (n, cout, h, w) and y.is_contiguous(memory_format=CL)
    wf, shift = nn_ops._folded(conv, bn)
    if second:
        shift = shift + rs                                           # (float32, as conv_bn_act forms the epilogue's operand)
    tag = 'wide eval (512, 128) %d->%d %dx%dx%d %s' % (cin, cout, n, h, w, 'shift+residual+relu' if second else 'shift+relu')
    ref, absum = nr.conv_fwd_ref(x, wf, shift=shift, residual=res, relu=True)
    _report(tag, nr.check(y, ref, nr.bf16_bound(ref, absum, nr.conv_accum_c(9 * cin)), tag))
    del ref, absum
    if second and h >= 600:
        p = nn_ops.avg_pool2x2(y)
        assert p.shape == (n, cout, h // 2, w // 2) and p.dtype == torch.bfloat16
        ref, bound = nr.avgpool_bound(y)
        tag = 'avg pool %dx%dx%dx%d -> %dx%d' % (n, cout, h, w, h // 2, w // 2)
        _report(tag, nr.check(p, ref, bound, tag))


# --------------------------------------------------------------------------------------------- the fused-BatchNorm c64 entry points
@pytest.mark.parametrize('shape', [(2, 21, 45), (32, 320, 100)])
def test_c64_statistics_finalize_and_transforming_convolutions(shape):
    """salsa_nn_conv3x3_c64_stats -> salsa_nn_bn_train_finalize -> salsa_nn_conv3x3_c64_xform_stats and
    salsa_nn_conv3x3_c64_wrw_xform with drop_p = 0 (public entry points without a caller in the package), against float64.

    finalize: mean / invstd / running statistics from the first convolution's partial table.  The table's float32 chain is
    c_s = (ceil(tiles / blocks) + 8) u of sum|x1| (the statistics test above); the kernel sums it in float64 and rounds mean
    and invstd once (u).  So |mean - ref| <= c_s mean|x1| + u |mean|, the variance moves by at most c_s (E x1^2 + 2 |mean| mean|x1|)
    and invstd by 0.5 invstd^3 of that (+ u invstd); the running statistics: the 8 u of
    test_batchnorm_train_forward_backward_at_bench_size plus momentum times those.

    The transforming kernels' operand: each landed 16-byte piece is rewritten in LDS (`transform` in conv_mfma.hip's
    conv3x3_c64_fwd_async_kernel; in registers between the global load and the LDS write in conv_c64_wrw.hip's conv3x3_c64_wrw_kernel<true>) as
    a = max(x1 * sc + sh, 0) in float32 with sc = fl(invstd * gamma), sh = fl(beta - mean * sc) (both fused multiply-adds),
    and rounds a to bf16 THERE, once, before any product (pack_bf16).  The reference forms a in float64 from the stored bf16
    x1, the kernel's own mean / invstd and that float32 sc / sh, rounds it to float32 and to bf16 the same way, and is a plain
    convolution / weight gradient of that operand, with the bounds of the untransformed kernels.
    Dropout (drop_p > 0) is not tested: its mask is a hash of the element index with no reference here."""
    from salsa_amd.crnn import nn_ops
    n, h, w = shape
    L = _lib()
    M = n * h * w
    tiles, tr = c64_config(L, n, h, w)
    assert (tiles, tr) == c64_plan(n, h, w)
    blocks = L.salsa_nn_conv3x3_c64_stats_blocks(n, h, w)
    assert blocks == (512 if tiles >= 512 else tiles)
    P, S = nn_ops._ptr, nn_ops._stream
    tag = 'c64 xform %dx%dx%d' % shape
    x0, w1, w2 = _act(n, 64, h, w, 80), _filt(64, 64, 3, 81), _filt(64, 64, 3, 82)
    part = torch.full((blocks, 2, 64), float('nan'), dtype=torch.float64, device=DEV)
    x1 = nn_ops._conv64(x0, w1, stats_part=part)
    g = torch.Generator(device=DEV).manual_seed(83)
    gamma, beta = torch.rand(64, device=DEV, generator=g) + 0.5, torch.randn(64, device=DEV, generator=g) * 0.5
    rm, rv = torch.randn(64, device=DEV, generator=g), torch.rand(64, device=DEV, generator=g) + 0.5
    rm0, rv0 = rm.double().clone(), rv.double().clone()
    save = torch.full((2, 64), float('nan'), device=DEV)
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    eps, mom = 1e-5, 0.1
    with torch.cuda.device(DEV):
        assert L.salsa_nn_bn_train_finalize(P(part), blocks, M, 64, eps, mom, P(rm), P(rv), P(save[0]), P(save[1]), P(count), S(x1)) == 0
    assert int(count) == 1
    xd = x1.double()
    mean = xd.mean(dim=(0, 2, 3))
    ex2 = (xd * xd).mean(dim=(0, 2, 3))
    mabs = xd.abs().mean(dim=(0, 2, 3))
    del xd
    var = ex2 - mean * mean
    invstd = 1.0 / torch.sqrt(var + eps)
    c_s = (-(-tiles // blocks) + 8) * nr.U32
    b_mean = c_s * mabs + nr.U32 * mean.abs()
    b_var = c_s * (ex2 + 2 * mean.abs() * mabs)
    _report(tag + ' finalize mean', nr.check(save[0], mean, b_mean, tag + ' mean'))
    _report(tag + ' finalize invstd', nr.check(save[1], invstd, 0.5 * invstd ** 3 * b_var + nr.U32 * invstd, tag + ' invstd'))
    unb = var * M / (M - 1)
    _report(tag + ' finalize running_mean', nr.check(rm, (1 - mom) * rm0 + mom * mean,
                                                     8 * nr.U32 * ((1 - mom) * rm0.abs() + mom * mean.abs()) + mom * b_mean, tag + ' running_mean'))
    _report(tag + ' finalize running_var', nr.check(rv, (1 - mom) * rv0 + mom * unb,
                                                    8 * nr.U32 * ((1 - mom) * rv0.abs() + mom * unb * (1 + mean ** 2 / var)) + mom * b_var,
                                                    tag + ' running_var'))
    # the operand the two kernels form from x1 and the kernel's own statistics
    sc = save[1] * gamma                                                               # float32 product, as the kernel's
    sh = (beta.double() - save[0].double() * sc.double()).float()                      # one rounding: a fused multiply-add
    a = (x1.double() * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)).clamp_(min=0).float().to(torch.bfloat16)
    a = a.contiguous(memory_format=CL)
    part2 = torch.full((blocks, 2, 64), float('nan'), dtype=torch.float64, device=DEV)
    y2 = torch.empty_like(x1, memory_format=CL)
    with torch.cuda.device(DEV):
        assert L.salsa_nn_conv3x3_c64_xform_stats(P(x1), P(w2), P(y2), P(part2), P(save[0]), P(save[1]), P(gamma), P(beta), 0.0, 0,
                                                  n, h, w, S(x1)) == 0
    ref, absum = nr.conv_fwd_ref(a, w2)
    _report(tag + ' conv(relu(bn(x1)))', nr.check(y2, ref, nr.bf16_bound(ref, absum, nr.conv_accum_c(9 * 64)), tag + ' forward'))
    del ref, absum
    yd = y2.double()
    _report(tag + ' stats sum', nr.check(part2[:, 0].sum(0), yd.sum(dim=(0, 2, 3)), c_s * yd.abs().sum(dim=(0, 2, 3)), tag + ' stats sum'))
    _report(tag + ' stats sumsq', nr.check(part2[:, 1].sum(0), (yd * yd).sum(dim=(0, 2, 3)), c_s * (yd * yd).sum(dim=(0, 2, 3)), tag + ' stats sumsq'))
    del yd
    gy = _act(n, 64, h, w, 84, offset=False)
    ref, absum = nr.conv_wgrad_ref(a, gy)
    for det in (False, True):
        nn_ops.set_deterministic(det, DEV)
        try:
            dw = torch.zeros((64, 3, 3, 64), dtype=torch.float32, device=DEV)
            with torch.cuda.device(DEV):
                assert L.salsa_nn_conv3x3_c64_wrw_xform(P(x1), P(gy), P(dw), P(save[0]), P(save[1]), P(gamma), P(beta), 0.0, 0,
                                                        n, h, w, S(x1)) == 0
            torch.cuda.synchronize()
        finally:
            nn_ops.set_deterministic(False, DEV)
        what = tag + ' dW of relu(bn(x1)) det=%d' % det
        _report(what, nr.check(dw.permute(0, 3, 1, 2), ref, nr.c64_wgrad_c(n, h, w) * absum + 1e-30, what))
