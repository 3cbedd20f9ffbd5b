"""The CRNN's hand-written kernels at the shapes the benchmark runs (batch 32), against float64 references with per-element
error bounds (tests/nn_reference.py).  Every case first asserts which instantiation it reaches: the kernels pick one from the
problem size, and the small shapes of tests/test_crnn_gpu.py never reach most of them.  Run alone:
python -m pytest -m gpu tests/test_nn_kernels_at_scale_gpu.py -q -s   (-s prints each case's max error / bound).

Two families of maps.  SALSA and the lin baseline features have 200 frequency bins (stem 640 x 200, then 320 x 100, 160 x 50,
80 x 25, 40 x 12); the mel baseline features (melspeciv 7 channels, melspecgcc 10) have 128 (640 x 128, 320 x 64, 160 x 32,
80 x 16, 40 x 8), and these reach other code, not only other sizes:

  kernel                      200-bin maps                         128-bin maps
  64 -> 64 (c64)              320 x 100: transposed, 8000 tiles    320 x 64: untransposed, 5120 tiles (~10 per workgroup)
  wide forward 128 -> 256     80 x 25: (512, 128)                  80 x 16: (256, 128)
  wide forward -> 512         40 x 12: (256, 128)                  40 x 8: (256, 64), 8 column blocks
  wide data gradient -> 128   80 x 25: (256, 128)                  80 x 16: (256, 64)
  wide weight gradient        W = 50 / 25 / 12: own instantiation  W = 32 / 16 / 8: the generic (W2C = 0) one, three buffers
  BatchNorm, 1 x 1 rows M     1 024 000 ... 15 360                 655 360 ... 10 240
  frequency mean              12 bins                              8 bins

The stem's 640-row maps in training and the maps of 60-s inference (4800 x 200 down to 300 x 12; the 1024-workgroup grid of the
64 -> 64 kernels, the fused pool, the 512-pixel wide tile at W = 12 / 8) are in tests/test_nn_kernels_full_res_gpu.py, with a
streamed float64 reference; only the frequency mean at 300 rows is a parameter here.
"""
import pytest
import torch

import nn_reference as nr
from test_nn_reference_cpu import MEL_STAGES, MEL_WIDE, WRW_IMMEDIATE_W, c64_config, c64_plan, config, wide_tile, wrw3

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
CL = torch.channels_last


def _lib():
    from salsa_amd import _lib
    return _lib.load()


def _report(what, ratio):
    print('%-58s max err / bound %.3g' % (what, ratio))
    return ratio


def _act(n, c, h, w, seed, offset=True):
    """bf16 channels-last activations; every third channel carries a mean of 1.5 - 3 (BatchNorm statistics and the
    cancellation in the convolutions' sums see a non-zero mean)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn((n, c, h, w), device=DEV, generator=g)
    if offset:
        mu = torch.zeros(c, device=DEV)
        mu[::3] = torch.linspace(1.5, 3.0, len(mu[::3]), device=DEV)
        x += mu.view(1, -1, 1, 1)
    return x.to(torch.bfloat16).contiguous(memory_format=CL)


def _filt(cout, cin, k, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    w = torch.randn((cout, cin, k, k), device=DEV, generator=g) * (2.0 / (k * k * cin)) ** 0.5
    return w.to(torch.bfloat16).contiguous(memory_format=CL)


# --------------------------------------------------------------------------------------------- wide 3x3, forward epilogues
# (N, Cin, Cout, H, W) -> the instantiation (pixels per tile, TN): all four, at bench layers
WIDE_FWD = [((32, 64, 128, 160, 50), (512, 128)),    # stage 2's first conv: a 512-pixel chunk is exactly MAX_XL_BYTES
            ((32, 256, 512, 40, 12), (256, 128)),    # stage 4's first conv
            ((32, 128, 64, 160, 50), (512, 64)),     # (the data gradient of 64 -> 128 as a convolution)
            ((32, 512, 256, 40, 12), (256, 64)),     # (the data gradient of 256 -> 512)
            ((32, 128, 256, 80, 16), (256, 128)),    # mel stage 3's first conv (80 x 25: (512, 128))
            ((32, 256, 512, 40, 8), (256, 64))]      # mel stage 4's first conv: Cout = 512 in 8 column blocks of 64


@pytest.mark.parametrize('shape,inst', WIDE_FWD)
def test_wide_conv_forward_stats_and_folded_epilogue(shape, inst):
    from salsa_amd.crnn import nn_ops
    n, cin, cout, h, w = shape
    L = _lib()
    assert L.salsa_nn_conv3x3_wide_supported(n, h, w, cin, cout) and config(L, n, h, w, cout) == inst == wide_tile(n, h, w, cout)
    x, wt = _act(n, cin, h, w, 1), _filt(cout, cin, 3, 2)
    ref, absum = nr.conv_fwd_ref(x, wt)
    c = nr.conv_accum_c(9 * cin)
    tag = '%s %d->%d %dx%dx%d' % (inst, cin, cout, n, h, w)
    # plain
    y = nn_ops._conv_wide(x, wt)
    _report('wide fwd ' + tag, nr.check(y, ref, nr.bf16_bound(ref, absum, c), 'wide fwd ' + tag))
    # training: the same output, and float64 partial sums of it (one row pair per pixel tile)
    blocks = L.salsa_nn_conv3x3_wide_stats_blocks(n, h, w, cin, cout)
    assert blocks == (n * h * w + inst[0] - 1) // inst[0]
    part = torch.full((blocks, 2, cout), float('nan'), dtype=torch.float64, device=DEV)
    ys = nn_ops._conv_wide(x, wt, stats_part=part)
    assert torch.equal(ys, y)
    yd = y.double()
    s_ref, q_ref = yd.sum(dim=(0, 2, 3)), (yd * yd).sum(dim=(0, 2, 3))
    # a tile's sums: float32 over its 64 pixels per wave (a pair add, two DPP steps, three shuffles: depth 7), then float64
    s_b = 8 * nr.U32 * yd.abs().sum(dim=(0, 2, 3))
    q_b = 8 * nr.U32 * (yd * yd).sum(dim=(0, 2, 3))
    _report('wide stats sum ' + tag, nr.check(part[:, 0].sum(0), s_ref, s_b, 'stats sum ' + tag))
    _report('wide stats sumsq ' + tag, nr.check(part[:, 1].sum(0), q_ref, q_b, 'stats sumsq ' + tag))
    # inference: folded shift + residual + ReLU before the single rounding
    g = torch.Generator(device=DEV).manual_seed(3)
    shift = torch.randn(cout, device=DEV, generator=g)
    res = _act(n, cout, h, w, 4, offset=False)
    yb = torch.empty_like(y)
    with torch.cuda.device(DEV):
        rc = L.salsa_nn_conv3x3_wide_bias_act(nn_ops._ptr(x), nn_ops._ptr(wt), nn_ops._ptr(shift), nn_ops._ptr(res), nn_ops._ptr(yb), 1,
                                              n, h, w, cin, cout, nn_ops._stream(x))
    assert rc == 0
    refb = (ref + shift.double().view(1, -1, 1, 1) + res.double()).clamp_(min=0)
    absb = absum + shift.double().abs().view(1, -1, 1, 1) + res.double().abs()
    _report('wide shift+res+relu ' + tag, nr.check(yb, refb, nr.bf16_bound(refb, absb, c), 'wide bias_act ' + tag))


# --------------------------------------------------------------------------------------------- wide 3x3, data gradients
BENCH_WIDE = [(64, 128, 160, 50), (128, 128, 160, 50), (128, 256, 80, 25), (256, 256, 80, 25), (256, 512, 40, 12), (512, 512, 40, 12)]


@pytest.mark.parametrize('layer', BENCH_WIDE + MEL_WIDE)
def test_wide_conv_data_gradient_of_every_bench_layer(layer):
    from salsa_amd.crnn import nn_ops
    cin, cout, h, w = layer
    n = 32
    L = _lib()
    inst = config(L, n, h, w, cin)
    assert L.salsa_nn_conv3x3_wide_supported(n, h, w, cout, cin) and inst == wide_tile(n, h, w, cin)
    gy, wt = _act(n, cout, h, w, 5), _filt(cout, cin, 3, 6)
    wf = nr.flip_filter(wt).contiguous(memory_format=CL)
    gx = nn_ops._conv_wide(gy, wf)
    ref, absum = nr.conv_fwd_ref(gy, wf)
    tag = '%s dgrad of %d->%d %dx%dx%d' % (inst, cin, cout, n, h, w)
    _report('wide ' + tag, nr.check(gx, ref, nr.bf16_bound(ref, absum, nr.conv_accum_c(9 * cout)), tag))


# --------------------------------------------------------------------------------------------- wide 3x3, weight gradients
WIDE_WRW = [((32, 64, 128, 160, 50), True), ((32, 128, 128, 160, 50), True),      # W = 50 (stage 2)
            ((32, 128, 256, 80, 25), True), ((32, 128, 256, 1, 25), False),        # W = 25
            ((32, 256, 512, 40, 12), True), ((32, 512, 512, 1, 12), False),        # W = 12
            ((32, 128, 128, 40, 33), True), ((32, 128, 128, 3, 40), False),        # the generic width
            ((32, 64, 128, 160, 32), True), ((32, 128, 256, 80, 16), True),        # the mel maps: generic width, three buffers
            ((32, 256, 512, 40, 8), True), ((32, 512, 512, 40, 8), True)]


@pytest.mark.parametrize('shape,three', WIDE_WRW)
def test_wide_conv_weight_gradient(shape, three):
    from salsa_amd.crnn import nn_ops
    n, cin, cout, h, w = shape
    L = _lib()
    assert L.salsa_nn_conv3x3_wide_wrw_supported(n, h, w, cin, cout) and wrw3(h, w) == three
    x, gy = _act(n, cin, h, w, 7), _act(n, cout, h, w, 8, offset=False)
    ref, absum = nr.conv_wgrad_ref(x, gy)
    for det in (False, True):
        nn_ops.set_deterministic(det, DEV)
        try:
            nn_ops.new_backward_generation(DEV)
            dw = nn_ops._conv_wide_wrw(x, gy).clone()
        finally:
            nn_ops.set_deterministic(False, DEV)
        tag = 'wide dW %s buffers %s W=%d %d->%d %dx%dx%d det=%d' % ('3' if three else '2', 'imm' if w in WRW_IMMEDIATE_W else 'generic',
                                                                   w, cin, cout, n, h, w, det)
        _report(tag, nr.check(dw, ref, nr.wide_wgrad_c(n, h, w, cin, cout) * absum, tag))


# --------------------------------------------------------------------------------------------- 64 -> 64 at 32 x 320 x {100, 64}
# (H, W) -> (tiles, transposed) of the forward / weight-gradient plan (4 x 32-pixel tiles, 512 persistent workgroups)
C64_MAPS = [((320, 100), (8000, 1)),       # SALSA / lin: transposed (10240 tiles untransposed)
            ((320, 64), (5120, 0))]        # mel: a tie, untransposed; each workgroup loops over ~10 tiles


@pytest.mark.parametrize('hw,geo', C64_MAPS, ids=['%dx%d' % hw for hw, _ in C64_MAPS])
def test_c64_conv_forward_and_gradients_at_bench_size(hw, geo):
    from salsa_amd.crnn import nn_ops
    n, (h, w) = 32, hw
    L = _lib()
    assert c64_config(L, n, h, w) == geo == c64_plan(n, h, w)
    blocks = L.salsa_nn_conv3x3_c64_stats_blocks(n, h, w)
    assert blocks == 512
    tag = '%dx%dx%d %s' % (n, h, w, 'transposed' if geo[1] else 'untransposed')
    x, gy, wt = _act(n, 64, h, w, 9), _act(n, 64, h, w, 10, offset=False), _filt(64, 64, 3, 11)
    y = nn_ops._conv64(x, wt)
    ref, absum = nr.conv_fwd_ref(x, wt)
    c = nr.conv_accum_c(9 * 64)
    _report('c64 fwd ' + tag, nr.check(y, ref, nr.bf16_bound(ref, absum, c), 'c64 fwd ' + tag))
    del ref, absum
    # training forward: the same output, and float64 partial sums of it per workgroup.  A sum's float32 chain: a row pair (1),
    # two DPP steps (2), then the lane's running sum over the workgroup's ceil(tiles / blocks) tiles, three shuffles (3)
    part = torch.full((blocks, 2, 64), float('nan'), dtype=torch.float64, device=DEV)
    ys = nn_ops._conv64(x, wt, stats_part=part)
    assert torch.equal(ys, y)
    yd = y.double()
    c_s = (-(-geo[0] // blocks) + 8) * nr.U32
    _report('c64 stats sum ' + tag, nr.check(part[:, 0].sum(0), yd.sum(dim=(0, 2, 3)), c_s * yd.abs().sum(dim=(0, 2, 3)), 'c64 stats sum'))
    _report('c64 stats sumsq ' + tag, nr.check(part[:, 1].sum(0), (yd * yd).sum(dim=(0, 2, 3)), c_s * (yd * yd).sum(dim=(0, 2, 3)),
                                               'c64 stats sumsq'))
    del yd, ys
    wf = nr.flip_filter(wt).contiguous(memory_format=CL)
    gx = nn_ops._conv64(gy, wf)
    ref, absum = nr.conv_fwd_ref(gy, wf)
    _report('c64 dgrad ' + tag, nr.check(gx, ref, nr.bf16_bound(ref, absum, c), 'c64 dgrad ' + tag))
    del ref, absum
    # the data gradient with the residual branch's gradient added in the epilogue (salsa_nn_conv3x3_c64_bias_act, zero shift)
    res = _act(n, 64, h, w, 12, offset=False)
    gxa = nn_ops._conv64(gy, wf, add=res)
    ref, absum = nr.conv_fwd_ref(gy, wf, residual=res)
    _report('c64 dgrad + residual ' + tag, nr.check(gxa, ref, nr.bf16_bound(ref, absum, c), 'c64 dgrad + residual ' + tag))
    del ref, absum, gxa, res
    dw = torch.zeros((64, 3, 3, 64), dtype=torch.float32, device=DEV)
    with torch.cuda.device(DEV):
        assert L.salsa_nn_conv3x3_c64_wrw(nn_ops._ptr(x), nn_ops._ptr(gy), nn_ops._ptr(dw), n, h, w, nn_ops._stream(x)) == 0
    ref, absum = nr.conv_wgrad_ref(x, gy)
    _report('c64 dW ' + tag, nr.check(dw.permute(0, 3, 1, 2), ref, nr.c64_wgrad_c(n, h, w) * absum, 'c64 dW ' + tag))


# --------------------------------------------------------------------------------------------- 1x1 shortcuts
# (Cin, Cout, H, W) of the three stride-2 blocks' shortcuts at batch 32
SHORTCUTS = [(64, 128, 160, 50), (128, 256, 80, 25), (256, 512, 40, 12),
             (64, 128, 160, 32), (128, 256, 80, 16), (256, 512, 40, 8)]            # (mel: M = 163 840 / 40 960 / 10 240)


@pytest.mark.parametrize('sc', SHORTCUTS)
def test_conv1x1_both_instantiations_and_weight_gradient_at_bench_size(sc):
    from salsa_amd.crnn import nn_ops
    cin, cout, h, w = sc
    n = 32
    M = n * h * w
    L = _lib()
    x, gy, wt = _act(n, cin, h, w, 12), _act(n, cout, h, w, 13, offset=False), _filt(cout, cin, 1, 14)
    # forward: Cout % 128 == 0 -> conv1x1_kernel<4>; the data gradient (Cout' = Cin) is <2> only for Cin = 64
    for name, a, f in (('fwd', x, wt), ('dgrad', gy, wt.transpose(0, 1).contiguous())):
        assert L.salsa_nn_conv1x1_supported(M, f.shape[1], f.shape[0])
        nt = 4 if f.shape[0] % 128 == 0 else 2
        y = nn_ops._conv1x1_hip(a, f)
        ref, absum = nr.conv_fwd_ref(a, f)
        tag = '1x1 %s <%d> %d->%d M=%d' % (name, nt, f.shape[1], f.shape[0], M)
        _report(tag, nr.check(y, ref, nr.bf16_bound(ref, absum, nr.conv_accum_c(f.shape[1])), tag))
    assert L.salsa_nn_conv1x1_wrw_supported(M, cin, cout)
    dw = torch.zeros((cout, cin), dtype=torch.float32, device=DEV)
    with torch.cuda.device(DEV):
        assert L.salsa_nn_conv1x1_wrw(nn_ops._ptr(x), nn_ops._ptr(gy), nn_ops._ptr(dw), M, cin, cout, nn_ops._stream(x)) == 0
    ref, absum = nr.conv_wgrad_ref(x, gy, k=1)
    tag = '1x1 dW %d->%d M=%d' % (cin, cout, M)
    _report(tag, nr.check(dw.view(cout, cin, 1, 1), ref, nr.conv1x1_wgrad_c(M, cin, cout) * absum, tag))


# --------------------------------------------------------------------------------------------- BatchNorm
# (C, H, W) of every stage at batch 32: M = 1 024 000 / 256 000 / 64 000 / 15 360 rows; mel: 655 360 / 163 840 / 40 960 / 10 240
BN_STAGES = [(64, 320, 100), (128, 160, 50), (256, 80, 25), (512, 40, 12)] + MEL_STAGES


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('pool', [False, True])
@pytest.mark.parametrize('stage', BN_STAGES)
def test_batchnorm_train_forward_backward_at_bench_size(stage, pool, dtype):
    from salsa_amd.crnn import nn_ops
    c, h, w = stage
    n = 32
    bf16 = dtype == torch.bfloat16
    assert _lib().salsa_nn_bn_supported(1 if bf16 else 0, n * h * w, c)
    x = _act(n, c, h, w, 15).to(dtype)
    res = _act(n, c, h, w, 16, offset=False).to(dtype)
    bn = nn_ops.BatchNormAct2d(c).to(DEV).train()
    g = torch.Generator(device=DEV).manual_seed(17)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, device=DEV, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(c, device=DEV, generator=g))
        bn.running_mean.copy_(torch.randn(c, device=DEV, generator=g))
        bn.running_var.copy_(torch.rand(c, device=DEV, generator=g) + 0.5)
    rm0, rv0 = bn.running_mean.double().clone(), bn.running_var.double().clone()
    xa, ra = x.clone().requires_grad_(True), res.clone().requires_grad_(True)
    y = bn.relu_pool(xa, residual=ra) if pool else bn(xa, residual=ra, relu=True)
    assert isinstance(y.grad_fn, (nn_ops._BnReluPool if pool else nn_ops._BnAct)._backward_cls)
    gy = _act(*y.shape[:1], c, *y.shape[2:], 18, offset=False).to(dtype)
    y.backward(gy)
    r = nr.bn_train_ref(x, bn.weight.detach(), bn.bias.detach(), bn.eps, residual=res, relu=True, pool=pool)
    fwd_c = 16 * nr.U32
    tag = 'bn %s %s C=%d M=%d' % ('pool' if pool else 'plain', 'bf16' if bf16 else 'fp32', c, r['M'])
    yb = fwd_c * (torch.nn.functional.avg_pool2d(r['fwd_abs'], 2) if pool else r['fwd_abs']) + (nr.BF16_REL * r['y'].abs() if bf16 else 0)
    _report(tag + ' y', nr.check(y, r['y'], yb, tag + ' y'))
    m = bn.momentum
    rm_ref = (1 - m) * rm0 + m * r['mean']
    rv_ref = (1 - m) * rv0 + m * r['unbiased']
    _report(tag + ' running_mean', nr.check(bn.running_mean, rm_ref, 8 * nr.U32 * ((1 - m) * rm0.abs() + m * r['mean'].abs()), tag))
    rv_b = 8 * nr.U32 * ((1 - m) * rv0.abs() + m * r['unbiased'] * (1 + r['mean'] ** 2 / r['var']))
    _report(tag + ' running_var', nr.check(bn.running_var, rv_ref, rv_b, tag))
    b = nr.bn_bwd_ref(r, bn.weight.detach(), gy, relu=True, pool=pool, fwd_c=fwd_c, bf16=bf16)
    keep = ~b['exempt']
    _report(tag + ' dx', nr.check(xa.grad.double()[keep], b['dx'][keep], b['b_dx'][keep], tag + ' dx'))
    _report(tag + ' dres', nr.check(ra.grad.double()[keep], b['dres'][keep], b['b_dres'][keep], tag + ' dres'))
    _report(tag + ' dgamma', nr.check(bn.weight.grad, b['dgamma'], b['b_dgamma'], tag + ' dgamma'))
    _report(tag + ' dbeta', nr.check(bn.bias.grad, b['dbeta'], b['b_dbeta'], tag + ' dbeta'))
    assert int(keep.sum()) >= keep.numel() * (1 - 1e-4)            # (few undecided ReLU masks)


# --------------------------------------------------------------------------------------------- frequency mean
@pytest.mark.parametrize('shape', [(32, 512, 40, 12), (32, 512, 40, 8), (32, 512, 300, 12), (32, 512, 300, 8)])    # (300 rows: 60-s inference)
def test_frequency_mean_forward_and_backward_at_bench_size(shape):
    """salsa_nn_freq_mean_fwd / _bwd as freq_mean_sequence calls them (time-major float32 buffer) against float64.  Forward: a
    sequential float32 sum of W terms ((W - 1) u of the sum of |x|), times fl(1 / W) (u of the mean for fl(1 / W), u for the
    product).  Backward: g fl(1 / W) rounded to bf16 -- bit for bit, and within 2^-8 + 2u of g / W."""
    from salsa_amd.crnn import nn_ops
    n, c, h, w = shape
    x = _act(n, c, h, w, 19).requires_grad_(True)
    y = nn_ops.freq_mean_sequence(x)
    assert y.shape == (n, h, c) and y.dtype == torch.float32 and y.transpose(0, 1).is_contiguous()     # the kernel's buffer
    xd = x.detach().double()
    ref = xd.mean(dim=3).transpose(1, 2)
    bound = ((w - 1) * xd.abs().sum(dim=3).transpose(1, 2) / w + 2 * ref.abs()) * nr.U32
    tag = 'freq mean %dx%dx%dx%d' % shape
    _report(tag + ' fwd', nr.check(y, ref, bound, tag + ' fwd'))
    g = torch.Generator(device=DEV).manual_seed(20)
    gy = torch.randn(y.shape, device=DEV, generator=g)
    y.backward(gy)
    want = (gy.double().transpose(1, 2).unsqueeze(3) / w).expand(shape)
    assert x.grad.shape == x.shape and x.grad.is_contiguous(memory_format=CL)
    _report(tag + ' bwd', nr.check(x.grad, want, (nr.BF16_REL + 2 * nr.U32) * want.abs(), tag + ' bwd'))
    inv = torch.ones((), device=DEV) / w                                 # fl(1 / W) in float32, as the kernel forms it
    assert torch.equal(x.grad, (gy.transpose(1, 2).unsqueeze(3) * inv).expand(shape).to(torch.bfloat16))   # (nearest even)


# --------------------------------------------------------------------------------------------- first layer at 32 x Cin x 640 x 128
def _features(n, cin, h, w, seed, kind):
    """float32 planar first-layer input: 'normalised' (every channel ~ N(0.3, 1)) or shaped like the unnormalised mel features
    (4 log-mel rows at -60 +- 12 dB, the IV / GCC channels in [-1, 1])"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    if kind == 'normalised':
        return torch.randn((n, cin, h, w), device=DEV, generator=g) + 0.3
    x = torch.empty((n, cin, h, w), device=DEV)
    x[:, :4] = torch.randn((n, 4, h, w), device=DEV, generator=g) * 12 - 60
    x[:, 4:] = torch.rand((n, cin - 4, h, w), device=DEV, generator=g) * 2 - 1
    return x


@pytest.mark.parametrize('cin', [7, 10])
def test_stem_forward_and_weight_gradient_at_mel_map(cin):
    """salsa_nn_conv3x3_stem, _stem_stats and _stem_wrw at 32 x Cin x 640 x 128 (melspeciv 7, melspecgcc 10 channels) on
    feature-shaped input, against conv_fwd_ref / conv_wgrad_ref on the bf16-rounded operands"""
    from salsa_amd.crnn import nn_ops
    from test_baseline_training_gpu import _stem_fwd, _stem_wrw_c, _w_from_filter
    n, h, w = 32, 640, 128
    L = _lib()
    g = torch.Generator(device=DEV).manual_seed(21 + cin)
    wq = nn_ops._stem_filter(torch.randn((64, cin, 3, 3), device=DEV, generator=g) * 0.2)
    assert tuple(wq.shape) == ((64, 10, 8) if cin <= 8 else (64, 9, 16)) and nn_ops._stem_wrw_hip(cin)
    nb = L.salsa_nn_conv3x3_stem_stats_blocks(n, h, w)
    assert nb == 1024                                                    # persistent over 10 240 tiles of 8 x 32 pixels
    x = _features(n, cin, h, w, 22 + cin, 'features')
    xq = x.bfloat16().float()
    tag = 'stem %d->64 %dx%dx%d' % (cin, n, h, w)
    y = _stem_fwd(x, wq)
    ref, absum = nr.conv_fwd_ref(xq, _w_from_filter(wq, cin))
    _report(tag + ' fwd', nr.check(y, ref, nr.bf16_bound(ref, absum, nr.conv_accum_c(wq.shape[1] * wq.shape[2])), tag + ' fwd'))
    del ref, absum
    yt, part = _stem_fwd(x, wq, stats=True)
    assert part.shape[0] == nb and torch.equal(yt, y)
    yd = y.double()
    torch.testing.assert_close(part.sum(0)[0], yd.sum(dim=(0, 2, 3)), rtol=1e-5, atol=1e-2)
    torch.testing.assert_close(part.sum(0)[1], (yd * yd).sum(dim=(0, 2, 3)), rtol=1e-5, atol=1e-2)
    del yd, yt, y
    gy = _act(n, 64, h, w, 23, offset=False)
    dw = torch.zeros((64, cin, 3, 3), device=DEV)
    with torch.cuda.device(DEV):
        assert L.salsa_nn_conv3x3_stem_wrw(nn_ops._ptr(x), x.stride(0), x.stride(1), nn_ops._ptr(gy), nn_ops._ptr(dw), n, cin, h, w,
                                           nn_ops._stream(x)) == 0
    ref, absum = nr.conv_wgrad_ref(xq, gy)
    _report(tag + ' dW', nr.check(dw, ref, _stem_wrw_c(n, h, w) * absum + 1e-30, tag + ' dW'))


def _stem_bn_ref(xq, wq, gam, bet, eps, gy):
    """float64 dW, dgamma, dbeta of relu(batch_norm(conv(xq, wq))) (training statistics) for the upstream gradient gy, clip by clip"""
    import torch.nn.functional as F
    n, cin, h, w = xq.shape
    wd = wq.reshape(64, cin * 9)
    conv = lambda i: wd @ F.unfold(xq[i:i + 1].double(), 3, padding=1)[0]       # (64, h w)
    s1 = torch.zeros(64, dtype=torch.float64, device=DEV)
    s2 = torch.zeros_like(s1)
    for i in range(n):
        z = conv(i)
        s1 += z.sum(1)
        s2 += (z * z).sum(1)
    cnt = n * h * w
    mu = s1 / cnt
    rstd = (s2 / cnt - mu * mu + eps).rsqrt()
    dgam, dbet = torch.zeros_like(s1), torch.zeros_like(s1)
    for i in range(n):
        xh = (conv(i) - mu[:, None]) * rstd[:, None]
        dz = gy[i].double().reshape(64, h * w) * ((gam[:, None] * xh + bet[:, None]) > 0)
        dgam += (dz * xh).sum(1)
        dbet += dz.sum(1)
    dW = torch.zeros((64, cin * 9), dtype=torch.float64, device=DEV)
    for i in range(n):
        cols = F.unfold(xq[i:i + 1].double(), 3, padding=1)[0]
        xh = (wd @ cols - mu[:, None]) * rstd[:, None]
        dz = gy[i].double().reshape(64, h * w) * ((gam[:, None] * xh + bet[:, None]) > 0)
        dzo = (gam * rstd)[:, None] * (dz - dbet[:, None] / cnt - xh * dgam[:, None] / cnt)
        dW += dzo @ cols.T
    return dW.reshape(64, cin, 3, 3), dgam, dbet


@pytest.mark.parametrize('kind', ['normalised', 'features'])
@pytest.mark.parametrize('cin', [7, 10])
def test_stem_batchnorm_backward_modes_at_mel_map(cin, kind, shape=(32, 640, 128)):
    """The first layer's weight gradient with its BatchNorm (+ ReLU) backward folded in at 32 x Cin x 640 x 128, in both modes --
    _bnf (the BatchNorm backward's reduction in the same pass, the training default) and _bn (reduction launch + coefficient
    table) -- against a float64 evaluation of the layer: no further from it than the two-node path (plain stem weight gradient
    after the separate BatchNorm backward) x 2, or 2e-3 of the scale; _bnf also no further than _bn x 2 (the rule of
    test_first_layer_reduce_fused_backward_at_bench_size_with_offset_inputs).  On feature-shaped input the bf16 rounding of the
    stored conv output dominates every path's distance from float64 (|mean| >> std), which makes that rule loose for _bn, so _bn
    -- the same dx formed on load instead of stored -- must also stay within 2e-3 of the scale of the two-node path."""
    from salsa_amd.crnn import nn_ops
    from test_baseline_training_gpu import _bn_step
    n, h, w = shape                      # (tests/test_nn_kernels_lite_maps_gpu.py calls this at 640 x 191)
    assert _lib().salsa_nn_bn_supported(1, n * h * w, 64) and nn_ops._stem_wrw_hip(cin)
    x = _features(n, cin, h, w, 24 + cin, kind)
    gy = _act(n, 64, h, w, 25, offset=False)
    saved = nn_ops.USE_STEM_FUSED_BWD, nn_ops.USE_STEM_BN_REDUCE_FUSED
    res = {}
    try:
        for key, fused, rf in (('bnf', True, True), ('bn', True, False), ('plain', False, True)):
            out, dW, dg, db, mods = _bn_step(cin, n, h, w, x, gy, fused, rf)      # (asserts the fused node iff fused)
            res[key] = (dW.double(), dg.double(), db.double())
            del out
        conv, bn = mods
        wq, gam, bet, eps = conv.weight.detach().bfloat16().double(), bn.weight.detach().double(), bn.bias.detach().double(), bn.eps
    finally:
        nn_ops.USE_STEM_FUSED_BWD, nn_ops.USE_STEM_BN_REDUCE_FUSED = saved
    want = _stem_bn_ref(x.bfloat16(), wq, gam, bet, eps, gy)
    err = {key: [float((a - b).abs().max()) / float(b.abs().max()) for a, b in zip(r, want)] for key, r in res.items()}
    tag = 'stem BN bwd %d->64 %dx%dx%d %s' % (cin, n, h, w, kind)
    for i, what in enumerate(('dW', 'dgamma', 'dbeta')):
        for key in ('bnf', 'bn'):
            bound = max(2.0 * err['plain'][i], 2e-3)
            _report('%s %s %s (plain %.3g)' % (tag, key, what, err['plain'][i]), err[key][i] / bound)
            assert err[key][i] <= bound, (tag, key, what, err)
        assert err['bnf'][i] <= max(2.0 * err['bn'][i], 2e-3), (tag, what, err)
        d = float((res['bn'][i] - res['plain'][i]).abs().max()) / float(res['plain'][i].abs().max())
        _report('%s bn - plain %s' % (tag, what), d / 2e-3)
        assert d <= 2e-3, (tag, what, d)


# --------------------------------------------------------------------------------------------- GRU
def _gru_case(H, T, B, seed):
    torch.manual_seed(seed)
    gru = torch.nn.GRU(512, H, num_layers=2, batch_first=True, bidirectional=True, dropout=0.0)
    x = torch.randn(B, T, 512)
    gy = torch.randn(B, T, 2 * H)
    return gru, x, gy


def _gru_run(gru, x, gy, half_weights):
    from salsa_amd.crnn import fused_gru
    g = gru.to(DEV).train()
    g.zero_grad()
    xa = x.to(DEV).requires_grad_(True)
    y = fused_gru.bigru_forward(g, xa, training=True, half_weights=half_weights)
    y.backward(gy.to(DEV))
    return y.detach().cpu(), [xa.grad.cpu()] + [p.grad.cpu() for p in g.parameters()]


def _names(gru):
    return ['y', 'dx'] + ['d' + n for n, _ in gru.named_parameters()]


@pytest.mark.parametrize('H', [64, 128, 256])
@pytest.mark.parametrize('TB', [(1, 1), (40, 32), (300, 32)])
def test_gru_scan_forward_and_every_gradient(H, TB):
    """the float32 streaming scans (salsa_gru_scan_fwd / _bwd) against nn.GRU in float64.  The yardstick is nn.GRU's own
    float32 evaluation on the CPU: the kernel's error may not exceed 16 times that (+ 2^-20 of the tensor's rms)."""
    T, B = TB
    gru, x, gy = _gru_case(H, T, B, 20 + H + T)
    y64, g64 = nr.gru_ref(gru, x, gy)
    import copy
    g32 = copy.deepcopy(gru)
    x32 = x.clone().requires_grad_(True)
    y32 = g32(x32)[0]
    y32.backward(gy)
    c32 = [y32.detach()] + [x32.grad] + [p.grad for p in g32.parameters()]
    got = _gru_run(gru, x, gy, False)
    got = [got[0]] + got[1]
    for name, a, b32, r in zip(_names(gru), got, c32, [y64] + g64):
        e = float((a.double() - r).abs().max())
        e32 = float((b32.double() - r).abs().max())
        bound = 16 * e32 + 2.0 ** -20 * float(r.pow(2).mean().sqrt())      # (0 for dW_hh at T = 1: h0 = 0, exactly)
        _report('gru H=%d T=%d B=%d %s' % (H, T, B, name), e / bound if bound > 0 else e)
        assert e <= bound, ('gru', H, T, B, name, e, e32)


def test_register_resident_gru_pair_at_bench_size():
    """salsa_gru_scan_fwd_regw / _bwd_regw (half_weights: W_hh and the recurrent h operand in float16) and the no-grad
    register-resident inference scan, T = 300, B = 32, against nn.GRU in float64 with W_hh rounded to float16: the residual
    difference is the float16 rounding of h in the recurrent products, 2^-11 relative per step."""
    from salsa_amd.crnn import fused_gru
    gru, x, gy = _gru_case(256, 300, 32, 30)
    r16 = lambda p: p.half().double()
    y64, g64 = nr.gru_ref(gru, x, gy, whh_round=r16)
    y, grads = _gru_run(gru, x, gy, True)
    for name, a, r in zip(_names(gru), [y] + grads, [y64] + g64):
        rms = float(r.pow(2).mean().sqrt())
        err = (a.double() - r).abs()
        ratio = float((err / (2e-3 * r.abs() + 2e-3 * rms)).max())
        _report('gru regw H=256 T=300 B=32 %s' % name, ratio)
        assert ratio <= 1, (name, float(err.max()), rms)
    with torch.no_grad():
        yi = fused_gru.bigru_forward(gru.to(DEV).eval(), x.to(DEV), training=False, half_weights=True).cpu()
    ratio = float(((yi.double() - y64).abs() / (2e-3 * y64.abs() + 2e-3 * float(y64.pow(2).mean().sqrt()))).max())
    _report('gru regw inference H=256 T=300 B=32 y', ratio)
    assert ratio <= 1
