"""The CRNN's hand-written kernels at the shapes the benchmark runs (batch 32), against float64 references with per-element
error bounds (tests/nn_reference.py).  Every case first asserts which instantiation it reaches: the kernels pick one from the
problem size, and the small shapes of tests/test_crnn_gpu.py never reach most of them.  Run alone:
python -m pytest -m gpu tests/test_nn_kernels_at_scale_gpu.py -q -s   (-s prints each case's max error / bound)."""
import pytest
import torch

import nn_reference as nr
from test_nn_reference_cpu import config, wide_tile

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
            ((32, 512, 256, 40, 12), (256, 64))]     # (the data gradient of 256 -> 512)


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


@pytest.mark.parametrize('layer', BENCH_WIDE)
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
def _wrw3(h, w):
    """conv_wide.hip's wrw3_supported restated: three tile buffers when a tile's x slots are few enough"""
    rc, ic = (127 + w - 1) // w, (127 + h * w - 1) // (h * w)
    xs = (127 + 2 * rc + (w + 2) * ic + 2 * (w + 2) + 3 + 15) & ~15
    lds = 3 * (xs * 64 + 128 * 256) + 3 * ((xs + 63) // 64) * 256 + 5 * 512 + 256
    return (xs + 63) // 64 + 2 <= 8 and xs // 16 <= 24 and lds <= 160 * 1024


WIDE_WRW = [((32, 64, 128, 160, 50), True), ((32, 128, 128, 160, 50), True),      # W = 50 (stage 2)
            ((32, 128, 256, 80, 25), True), ((32, 128, 256, 1, 25), False),        # W = 25
            ((32, 256, 512, 40, 12), True), ((32, 512, 512, 1, 12), False),        # W = 12
            ((32, 128, 128, 40, 33), True), ((32, 128, 128, 3, 40), False)]        # the generic width


@pytest.mark.parametrize('shape,three', WIDE_WRW)
def test_wide_conv_weight_gradient(shape, three):
    from salsa_amd.crnn import nn_ops
    n, cin, cout, h, w = shape
    L = _lib()
    assert L.salsa_nn_conv3x3_wide_wrw_supported(n, h, w, cin, cout) and _wrw3(h, w) == three
    x, gy = _act(n, cin, h, w, 7), _act(n, cout, h, w, 8, offset=False)
    ref, absum = nr.conv_wgrad_ref(x, gy)
    for det in (False, True):
        nn_ops.set_deterministic(det, DEV)
        try:
            nn_ops.new_backward_generation(DEV)
            dw = nn_ops._conv_wide_wrw(x, gy).clone()
        finally:
            nn_ops.set_deterministic(False, DEV)
        tag = 'wide dW %s buffers W=%d %d->%d %dx%dx%d det=%d' % ('3' if three else '2', w, cin, cout, n, h, w, det)
        _report(tag, nr.check(dw, ref, nr.wide_wgrad_c(n, h, w, cin, cout) * absum, tag))


# --------------------------------------------------------------------------------------------- 64 -> 64 at 32 x 320 x 100
def test_c64_conv_forward_and_gradients_at_bench_size():
    from salsa_amd.crnn import nn_ops
    n, h, w = 32, 320, 100
    L = _lib()
    x, gy, wt = _act(n, 64, h, w, 9), _act(n, 64, h, w, 10, offset=False), _filt(64, 64, 3, 11)
    y = nn_ops._conv64(x, wt)
    ref, absum = nr.conv_fwd_ref(x, wt)
    c = nr.conv_accum_c(9 * 64)
    _report('c64 fwd 32x320x100', nr.check(y, ref, nr.bf16_bound(ref, absum, c), 'c64 fwd'))
    del ref, absum
    wf = nr.flip_filter(wt).contiguous(memory_format=CL)
    gx = nn_ops._conv64(gy, wf)
    ref, absum = nr.conv_fwd_ref(gy, wf)
    _report('c64 dgrad 32x320x100', nr.check(gx, ref, nr.bf16_bound(ref, absum, c), 'c64 dgrad'))
    del ref, absum
    dw = torch.zeros((64, 3, 3, 64), dtype=torch.float32, device=DEV)
    with torch.cuda.device(DEV):
        assert L.salsa_nn_conv3x3_c64_wrw(nn_ops._ptr(x), nn_ops._ptr(gy), nn_ops._ptr(dw), n, h, w, nn_ops._stream(x)) == 0
    ref, absum = nr.conv_wgrad_ref(x, gy)
    _report('c64 dW 32x320x100', nr.check(dw.permute(0, 3, 1, 2), ref, nr.c64_wgrad_c(n, h, w) * absum, 'c64 dW'))


# --------------------------------------------------------------------------------------------- 1x1 shortcuts
# (Cin, Cout, H, W) of the three stride-2 blocks' shortcuts at batch 32
SHORTCUTS = [(64, 128, 160, 50), (128, 256, 80, 25), (256, 512, 40, 12)]


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
# (C, H, W) of every stage at batch 32: M = 1 024 000 / 256 000 / 64 000 / 15 360 rows
BN_STAGES = [(64, 320, 100), (128, 160, 50), (256, 80, 25), (512, 40, 12)]


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
