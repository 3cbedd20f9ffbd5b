"""GPU tests of training the CRNN on the baseline features: the 16-channel first-layer kernels (salsa_nn_conv3x3_stem* with
9 <= Cin <= 16; weight gradient up to 14) against float64 references with per-element bounds (tests/nn_reference.py), the GCC
augmentation kernel (salsa_augment_gcc_batch) and the IV recipes on the reference's own draws (golden g22), a full 10-channel
training step without MIOpen, the 10-channel model against the reference model (g23), and the baseline feature bank."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from nn_reference import U32, bf16_bound, check, conv_accum_c, conv_fwd_ref, conv_wgrad_ref

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')


def _input(n, cin, h, w, g, crop=0):
    """float32 planar features; crop > 0: a time-cropped view (rows contiguous, strides of the larger tensor)"""
    x = torch.randn((n, cin, h + crop, w), device=DEV, generator=g)
    return x[:, :, crop // 2:crop // 2 + h] if crop else x


def _stem_fwd(x, wq, shift=None, relu=False, stats=False):
    from salsa_amd import _lib
    from salsa_amd.crnn import nn_ops
    L = _lib.load()
    n, cin, h, w = x.shape
    y = torch.empty((n, 64, h, w), dtype=torch.bfloat16, device=DEV, memory_format=torch.channels_last)
    if stats:
        nb = L.salsa_nn_conv3x3_stem_stats_blocks(n, h, w)
        part = torch.full((nb * 128,), float('nan'), dtype=torch.float64, device=DEV)
        rc = L.salsa_nn_conv3x3_stem_stats(nn_ops._ptr(x), x.stride(0), x.stride(1), nn_ops._ptr(wq), nn_ops._ptr(y), nn_ops._ptr(part),
                                           n, cin, h, w, nn_ops._stream(x))
        assert rc == 0
        return y, part.view(nb, 2, 64)
    rc = L.salsa_nn_conv3x3_stem(nn_ops._ptr(x), x.stride(0), x.stride(1), nn_ops._ptr(wq), nn_ops._ptr(shift), nn_ops._ptr(y), int(relu),
                                 n, cin, h, w, nn_ops._stream(x))
    assert rc == 0
    return y


def _w_from_filter(wq, cin):
    """the bf16 filter values the kernel multiplies, back in (64, cin, 3, 3)"""
    return wq.float()[:, :9, :cin].reshape(64, 3, 3, cin).permute(0, 3, 1, 2).contiguous()


FWD_CASES = [(1, 9, 9, 33, 0), (2, 10, 17, 5, 3), (3, 14, 40, 70, 5), (2, 16, 8, 32, 0), (1, 10, 1, 1, 0), (4, 16, 23, 47, 2)]


@pytest.mark.parametrize('n,cin,h,w,crop', FWD_CASES)
def test_stem16_forward_epilogues_against_float64(n, cin, h, w, crop):
    """salsa_nn_conv3x3_stem / _stats at 9 <= Cin <= 16 ([64][9][16] filter): plain, folded shift + ReLU and the statistics
    launch against conv_fwd_ref on the bf16-rounded operands, per element within bf16_bound; edge tiles, a time-cropped view."""
    from salsa_amd.crnn import nn_ops
    g = torch.Generator(device=DEV).manual_seed(100 + cin)
    x = _input(n, cin, h, w, g, crop)
    wq = nn_ops._stem_filter(torch.randn((64, cin, 3, 3), device=DEV, generator=g) * 0.2)
    assert tuple(wq.shape) == (64, 9, 16)
    xq, wf = x.bfloat16().float(), _w_from_filter(wq, cin)
    c = conv_accum_c(16 * 9)
    ref, absum = conv_fwd_ref(xq, wf)
    y = _stem_fwd(x, wq)
    check(y.float(), ref, bf16_bound(ref, absum, c), 'stem16 plain cin=%d' % cin)
    shift = torch.randn(64, device=DEV, generator=g) * 0.5
    ref_s, absum_s = conv_fwd_ref(xq, wf, shift=shift, relu=True)
    ys = _stem_fwd(x, wq, shift, relu=True)
    check(ys.float(), ref_s, bf16_bound(ref_s, absum_s, c), 'stem16 shift+relu cin=%d' % cin)
    yt, part = _stem_fwd(x, wq, stats=True)
    assert torch.equal(yt, y)
    yf = y.double()
    torch.testing.assert_close(part.sum(0)[0], yf.sum(dim=(0, 2, 3)), rtol=1e-5, atol=1e-3)
    torch.testing.assert_close(part.sum(0)[1], (yf * yf).sum(dim=(0, 2, 3)), rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize('w', [128, 200])
def test_stem16_forward_at_bench_shapes(w):
    """(32, 10, 640, 128) and (32, 10, 640, 200): the GCC bench shapes, plain and statistics epilogues, every element."""
    from salsa_amd.crnn import nn_ops
    g = torch.Generator(device=DEV).manual_seed(7)
    x = _input(32, 10, 640, w, g)
    wq = nn_ops._stem_filter(torch.randn((64, 10, 3, 3), device=DEV, generator=g) * 0.2)
    y = _stem_fwd(x, wq)
    ref, absum = conv_fwd_ref(x.bfloat16().float(), _w_from_filter(wq, 10))
    r = check(y.float(), ref, bf16_bound(ref, absum, conv_accum_c(16 * 9)), 'stem16 bench w=%d' % w)
    del ref, absum
    yt, part = _stem_fwd(x, wq, stats=True)
    assert torch.equal(yt, y)
    yf = y.double()
    torch.testing.assert_close(part.sum(0)[0], yf.sum(dim=(0, 2, 3)), rtol=1e-5, atol=1e-2)
    print('stem16 forward 32x10x640x%d: max err / bound %.3g' % (w, r))


def _stem_wrw_c(n, h, w):
    """c for salsa_nn_conv3x3_stem_wrw: nb = min(tiles, 1280) persistent workgroups of 4 x 32-pixel tiles, an MFMA update per
    16 pixels (8 per tile, + 16 in the MFMA), then the nb partials added (slabs in order or atomics)."""
    tiles = n * math.ceil(h / 4) * math.ceil(w / 32)
    nb = min(tiles, 1280)
    return (math.ceil(tiles / nb) * 8 + 16 + nb) * U32


WRW_CASES = [(1, 9, 9, 33, 0), (2, 10, 17, 5, 3), (3, 14, 40, 70, 5), (2, 12, 8, 32, 0), (32, 10, 640, 128, 0), (32, 10, 640, 200, 0)]


@pytest.mark.parametrize('n,cin,h,w,crop', WRW_CASES)
def test_stem16_weight_gradient_against_float64(n, cin, h, w, crop):
    """salsa_nn_conv3x3_stem_wrw at 9 <= Cin <= 14 (two 64-column blocks) against conv_wgrad_ref, per element; the deterministic
    default twice gives identical bits; Cin = 15 / 16 are refused (the stated cap)."""
    from salsa_amd import _lib
    from salsa_amd.crnn import nn_ops
    L = _lib.load()
    nn_ops.new_backward_generation(DEV)                                  # (selects the deterministic default, SALSA_DETERMINISTIC=1)
    assert L.salsa_nn_get_deterministic() == 1
    g = torch.Generator(device=DEV).manual_seed(200 + cin)
    x = _input(n, cin, h, w, g, crop)
    gy = torch.randn((n, 64, h, w), device=DEV, generator=g).bfloat16().contiguous(memory_format=torch.channels_last)
    outs = []
    for _ in range(2):
        dw = torch.zeros((64, cin, 3, 3), device=DEV)
        rc = L.salsa_nn_conv3x3_stem_wrw(nn_ops._ptr(x), x.stride(0), x.stride(1), nn_ops._ptr(gy), nn_ops._ptr(dw), n, cin, h, w,
                                         nn_ops._stream(x))
        assert rc == 0
        outs.append(dw)
    assert torch.equal(outs[0], outs[1])
    ref, absum = conv_wgrad_ref(x.bfloat16().float(), gy.float())
    r = check(outs[0], ref, _stem_wrw_c(n, h, w) * absum + 1e-30, 'stem16 wrw cin=%d %dx%dx%d' % (cin, n, h, w))
    print('stem16 wrw cin=%d %dx%dx%d: max err / bound %.3g' % (cin, n, h, w, r))
    for bad in (15, 16):
        xb = _input(1, bad, 8, 32, g)
        assert L.salsa_nn_conv3x3_stem_wrw(nn_ops._ptr(xb), xb.stride(0), xb.stride(1), nn_ops._ptr(gy), nn_ops._ptr(outs[0]), 1, bad,
                                           8, 32, nn_ops._stream(xb)) == -1


def _bn_step(cin, n, h, w, x, gy, fused, reduce_fused):
    """relu(bn(conv(x))) forward + backward in training with the switches given -> (out, dW, dgamma, dbeta, mods)"""
    from salsa_amd.crnn import nn_ops
    nn_ops.USE_STEM_FUSED_BWD, nn_ops.USE_STEM_BN_REDUCE_FUSED = fused, reduce_fused
    torch.manual_seed(5)
    conv, bn = nn_ops.Conv3x3(cin, 64, 3, padding=1, bias=False).to(DEV), nn_ops.BatchNormAct2d(64).to(DEV)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        out = nn_ops.conv_bn_act(conv, bn, x)
    assert isinstance(out.grad_fn, nn_ops._StemConvBnRelu._backward_cls) == fused
    out.backward(gy)
    return out.detach(), conv.weight.grad.clone(), bn.weight.grad.clone(), bn.bias.grad.clone(), (conv, bn)


@pytest.mark.parametrize('n,cin,h,w', [(2, 10, 40, 70), (1, 9, 9, 33), (3, 14, 17, 5), (4, 10, 64, 200)])
def test_stem16_batchnorm_weight_gradient_modes_against_float64(n, cin, h, w):
    """The first layer's weight gradient with the BatchNorm (+ ReLU) behind it, in both fused modes -- _bnf (the BatchNorm
    backward's reduction folded in, MODE 2, the training default) and _bn (dx formed on the fly, MODE 1) -- against the two-node
    path (plain stem16 wrw + separate BatchNorm backward) to 2e-3 of max |dW| (as for 7 channels in test_crnn_gpu.py), and
    all of them against a float64 evaluation of the layer: no further from it than the first layer on MIOpen (SALSA_HIP_STEM16=0)
    x2, or 2e-3 of the scale.  _bnf twice gives the same bits."""
    import torch.nn.functional as F
    from salsa_amd.crnn import nn_ops
    saved = nn_ops.USE_STEM_FUSED_BWD, nn_ops.USE_STEM_BN_REDUCE_FUSED, nn_ops.USE_HIP_STEM16
    g = torch.Generator(device=DEV).manual_seed(300 + cin)
    x = _input(n, cin, h, w, g)
    gy = torch.randn((n, 64, h, w), device=DEV, generator=g).bfloat16().contiguous(memory_format=torch.channels_last)
    try:
        res = {}
        for key, fused, rf in (('bnf', True, True), ('bn', True, False), ('plain', False, True), ('miopen', False, True)):
            nn_ops.USE_HIP_STEM16 = key != 'miopen'
            out, dW, dg, db, mods = _bn_step(cin, n, h, w, x, gy, fused, rf)
            res[key] = (dW.double(), dg.double(), db.double())
            if key == 'bnf':
                _, dW2, dg2, db2, _ = _bn_step(cin, n, h, w, x, gy, True, True)
                assert torch.equal(dW, dW2) and torch.equal(dg, dg2) and torch.equal(db, db2)
        conv, bn = mods
        wq, gam, bet, eps = conv.weight.detach().bfloat16().double(), bn.weight.detach().double(), bn.bias.detach().double(), bn.eps
    finally:
        nn_ops.USE_STEM_FUSED_BWD, nn_ops.USE_STEM_BN_REDUCE_FUSED, nn_ops.USE_HIP_STEM16 = saved
    for key in ('bnf', 'bn'):
        for a, b in zip(res[key], res['plain']):
            torch.testing.assert_close(a, b, rtol=2e-3, atol=2e-3 * float(b.abs().max()) + 1e-6, msg=key)
    xq = x.bfloat16().double()
    z = F.conv2d(xq, wq, padding=1)
    cnt = n * h * w
    mu = z.mean(dim=(0, 2, 3))
    var = (z * z).mean(dim=(0, 2, 3)) - mu * mu
    rstd = (var + eps).rsqrt()
    xh = (z - mu[None, :, None, None]) * rstd[None, :, None, None]
    dz = gy.double() * ((gam[None, :, None, None] * xh + bet[None, :, None, None]) > 0)
    dgam, dbet = (dz * xh).sum(dim=(0, 2, 3)), dz.sum(dim=(0, 2, 3))
    dzo = (gam * rstd)[None, :, None, None] * (dz - dbet[None, :, None, None] / cnt - xh * dgam[None, :, None, None] / cnt)
    dW = torch.einsum('npq,ncq->pc', dzo.reshape(n, 64, h * w), F.unfold(xq, 3, padding=1)).reshape(64, cin, 3, 3)
    err = {key: [float((got - want).abs().max()) / float(want.abs().max()) for got, want in zip(r, (dW, dgam, dbet))]
           for key, r in res.items()}
    print('stem16 BN-backward modes, max err / scale (dW, dgamma, dbeta):', {k: ['%.3g' % e for e in v] for k, v in err.items()})
    for key in ('bnf', 'bn', 'plain'):
        for e, e_miopen, what in zip(err[key], err['miopen'], ('dW', 'dgamma', 'dbeta')):
            assert e <= max(2.0 * e_miopen, 2e-3), (key, what, e, e_miopen)


def test_stem16_is_routed_and_switchable():
    """Conv3x3(10, 64) under bf16 autocast takes the stem kernels (forward and weight gradient, no MIOpen call); SALSA_HIP_STEM16=0
    (nn_ops.USE_HIP_STEM16 = False) sends it back to torch; Cin = 8 keeps its weight gradient on MIOpen as before."""
    from salsa_amd.crnn import nn_ops
    conv = nn_ops.Conv3x3(10, 64, 3, padding=1, bias=False).to(DEV)
    x = torch.randn((2, 10, 16, 40), device=DEV)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        assert conv._stem_eligible(x)
        y = conv(x)
    assert isinstance(y.grad_fn, nn_ops._Conv3x3Stem._backward_cls)
    saved = nn_ops.USE_HIP_STEM16
    nn_ops.USE_HIP_STEM16 = False
    try:
        with torch.autocast('cuda', dtype=torch.bfloat16):
            assert not conv._stem_eligible(x)
            y2 = conv(x)
        assert not isinstance(y2.grad_fn, nn_ops._Conv3x3Stem._backward_cls)
    finally:
        nn_ops.USE_HIP_STEM16 = saved
    assert nn_ops._stem_wrw_hip(10) and nn_ops._stem_wrw_hip(14) and nn_ops._stem_wrw_hip(7)
    assert not nn_ops._stem_wrw_hip(8) and not nn_ops._stem_wrw_hip(15) and not nn_ops._stem_wrw_hip(16)


@pytest.mark.parametrize('fmt,ft', [('foa', 'linspeciv'), ('foa', 'melspeciv'), ('mic', 'linspecgcc'), ('mic', 'melspecgcc')])
def test_baseline_augmentation_kernels_reproduce_the_reference_samples(fmt, ft):
    """Golden g22 THROUGH the HIP kernels: for each of 48 seeds the reference's own draws (np.random.seed(s), consumed in its call
    order by reference_draws) become the kernel's parameters -- salsa_augment_gcc_batch for the GCC types, salsa_augment_batch
    (FOA swap + cutout with 3 zero rows) for IV; features hash to what the reference produced, targets likewise."""
    import hashlib
    from salsa_amd.augment import apply_augment_hip, reference_draws, swap_targets
    meta, a = load_golden('g22_baseline_augment')
    x = torch.from_numpy(a['x10' if ft.endswith('gcc') else 'x7'])[None].to(DEV).contiguous()
    y_doa = torch.from_numpy(a['y_doa'])[None].to(DEV)
    T, F = x.shape[2:]
    changed = cut = 0
    for s, (hx, hd) in zip(meta['seeds'], meta['sha'][ft]):
        np.random.seed(s)

        def minmax_after(d):
            y = apply_augment_hip(x, d, fmt, ft)
            return float(y.min()), float(y.max())
        d = reference_draws(np.random, T, F, fmt, minmax_after, feature_type=ft)
        xo = apply_augment_hip(x, d, fmt, ft)[0].cpu().numpy()
        do = swap_targets(y_doa, d['m'].to(DEV), fmt)[0].cpu().numpy()
        if ('%s_x_%d' % (ft, s)) in a:
            assert np.array_equal(xo, a['%s_x_%d' % (ft, s)]) and np.array_equal(do, a['%s_doa_%d' % (ft, s)]), (ft, s)
        assert hashlib.sha256(np.ascontiguousarray(xo).tobytes()).hexdigest() == hx, (ft, s)
        assert hashlib.sha256(np.ascontiguousarray(do).tobytes()).hexdigest() == hd, (ft, s)
        changed += not np.array_equal(xo, a['x10' if ft.endswith('gcc') else 'x7'])
        cut += int(d['h'].sum() > 0)
    assert changed > len(meta['seeds']) // 2 and cut > 8, (changed, cut)


def test_gcc_augmentation_kernel_matches_torch_on_a_cropped_batch():
    """augment_batch(feature_type='melspecgcc') on a time-cropped CUDA batch (HIP kernel) = apply_augment_torch on the same draws."""
    from salsa_amd.augment import apply_augment_hip, apply_augment_torch, draw_augment, swap_targets
    g = torch.Generator(device=DEV).manual_seed(8)
    x = torch.randn((32, 10, 700, 128), device=DEV, generator=g)[:, :, 30:670]
    y_doa = torch.randn((32, 80, 36), device=DEV, generator=g)
    d = draw_augment(32, 640, 128, 'mic', torch.Generator().manual_seed(2), feature_type='melspecgcc')
    got = apply_augment_hip(x, d, 'mic', 'melspecgcc')
    want, yw = apply_augment_torch(x, y_doa, d, 'mic', feature_type='melspecgcc')
    assert torch.equal(got, want)
    assert torch.equal(swap_targets(y_doa, d['m'].to(DEV), 'mic'), yw)


def test_ten_channel_training_step_calls_no_miopen_convolution(monkeypatch):
    """One full training step on a (32, 10, 640, 128) GCC batch: no torch.nn.Conv2d._conv_forward and no
    aten.convolution_backward call; loss and gradients against the same step with SALSA_HIP_STEM16=0 (the first layer on MIOpen)
    under the bf16 rules of test_crnn_gpu.py's HIP vs torch comparison: both losses within 1 % of the float32 step's, and the
    gradients' relative errors against the float32 step no larger than the MIOpen path's (median x1.25 + 0.02, max x1.5 + 0.05;
    the first layer's own gradient likewise)."""
    from salsa_amd.crnn import nn_ops
    from salsa_amd.crnn.loss import seld_loss
    from salsa_amd.crnn.testing import dropout_off
    from salsa_amd.crnn.train import Trainer, synthetic_batch
    calls = {'fwd': 0, 'bwd': 0}
    real_fwd = torch.nn.Conv2d._conv_forward

    def fwd(self, *a, **k):
        calls['fwd'] += 1
        return real_fwd(self, *a, **k)

    class CountingOp:                                                  # the op packet, counted when called (torch reads its overloads)
        def __init__(self, op):
            self.op = op

        def __call__(self, *a, **k):
            calls['bwd'] += 1
            return self.op(*a, **k)

        def __getattr__(self, name):
            return getattr(self.op, name)
    monkeypatch.setattr(torch.nn.Conv2d, '_conv_forward', fwd)
    monkeypatch.setattr(torch.ops.aten, 'convolution_backward', CountingOp(torch.ops.aten.convolution_backward))
    x, sed, doa = synthetic_batch(32, DEV, seed=4, n_frames=640, n_freq=128, n_channels=10)

    def step(hip16, amp=torch.bfloat16):
        monkeypatch.setattr(nn_ops, 'USE_HIP_STEM16', hip16)
        calls['fwd'] = calls['bwd'] = 0
        tr = Trainer(DEV, total_steps=10, n_input_channels=10, amp_dtype=amp)
        tr.model.train()
        with dropout_off(tr.raw_model):
            with torch.autocast('cuda', dtype=torch.bfloat16, enabled=amp is not None):
                pred = tr.model(tr._input_layout(x))
            loss = seld_loss(pred, sed, doa)[0]
            loss.backward()
        torch.cuda.synchronize()
        grads = {k: p.grad.float().clone() for k, p in tr.raw_model.named_parameters() if p.grad is not None}
        return float(loss.detach()), grads, dict(calls)

    loss_on, g_on, c_on = step(True)
    assert c_on == {'fwd': 0, 'bwd': 0}, c_on
    loss_off, g_off, c_off = step(False)
    assert c_off['fwd'] > 0, c_off                                               # (the counter does see the MIOpen path)
    loss_ref, g_ref, _ = step(True, None)                                        # float32 everywhere: the yardstick
    print('loss stem16 / MIOpen stem / float32', loss_on, loss_off, loss_ref)
    assert abs(loss_on - loss_ref) < 1e-2 * max(1.0, abs(loss_ref)) and abs(loss_off - loss_ref) < 1e-2 * max(1.0, abs(loss_ref))
    assert set(g_on) == set(g_off) == set(g_ref)
    # test_crnn_gpu.py's rule: every bf16 path is tens of percent from float32 per tensor at random initialisation; the HIP
    # first layer must be no noisier than the MIOpen one
    e_on = sorted((g_on[k] - g_ref[k]).norm().item() / (g_ref[k].norm().item() + 1e-12) for k in g_ref)
    e_off = sorted((g_off[k] - g_ref[k]).norm().item() / (g_ref[k].norm().item() + 1e-12) for k in g_ref)
    mid = len(e_on) // 2
    e1 = [(g[k] - g_ref[k]).norm().item() / g_ref[k].norm().item() for g in (g_on, g_off) for k in ('encoder.stem.conv1.weight',)]
    print('gradient error vs float32, median / max: stem16 %.3f / %.3f   MIOpen stem %.3f / %.3f; conv1: %.3f / %.3f'
          % (e_on[mid], e_on[-1], e_off[mid], e_off[-1], e1[0], e1[1]))
    assert e_on[mid] <= 1.25 * e_off[mid] + 2e-2 and e_on[-1] <= 1.5 * e_off[-1] + 5e-2
    assert e1[0] <= 1.5 * e1[1] + 5e-2


def test_ten_channel_model_on_the_gpu_matches_the_reference_model():
    """g23 on the GPU: float32 forward at the g9 GPU test's tolerance, and the bf16 eval forward (the 16-channel stem kernel with
    the folded BatchNorm) at the bf16 tolerance of test_crnn_gpu.py's HIP vs torch eval comparison."""
    from salsa_amd.crnn import SeldCRNN
    from salsa_amd.crnn.testing import seeded_fill
    meta, a = load_golden('g23_crnn10')
    m = SeldCRNN(n_input_channels=10)
    seeded_fill(m, meta['weight_seed'])
    m = m.to(DEV).eval()
    x = torch.randn(*meta['input_shape'], generator=torch.Generator().manual_seed(meta['input_seed'])).to(DEV)
    with torch.no_grad():
        out = m(x)
    np.testing.assert_allclose(out['event_frame_logit'].cpu().numpy(), a['event_frame_logit'], rtol=2e-3, atol=2e-4)
    np.testing.assert_allclose(out['doa_frame_output'].cpu().numpy(), a['doa_frame_output'], rtol=2e-3, atol=2e-4)
    m = m.to(memory_format=torch.channels_last)
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
        assert m.encoder.stem.conv1._stem_eligible(x)
        out = m(x)
    for k in ('event_frame_logit', 'doa_frame_output'):
        got = out[k].float().cpu().numpy()
        print('g23 bf16 %s: max |err| %.3g' % (k, float(np.abs(got - a[k]).max())))
        np.testing.assert_allclose(got, a[k], rtol=5e-2, atol=5e-2)


def test_baseline_bank_normalises_every_channel(tmp_path):
    """A bank of 10-channel feature files with the reference's (10, 1, F) scaler normalises all 10 channels exactly as
    database.py:197-202 does ((x - mean) / std in float32); a bank fed audio through a BaselineExtractor fits a (C, 1, F) scaler
    over all channels (compute_scaler of the baseline features); a SALSA bank still covers 4."""
    from salsa_amd import io as sio
    from salsa_amd.baseline_features import BaselineExtractor
    from salsa_amd.dataset import GpuFeatureBank
    from salsa_amd.extractor import SalsaExtractor
    from salsa_amd.synth import synth_clip
    rng = np.random.RandomState(3)
    files = []
    for i in range(3):
        f = str(tmp_path / ('clip%d.h5' % i))
        sio.save_arrays(f, feature=(rng.randn(10, 640 + 8 * i, 128) * 3 + 1).astype(np.float32))
        files.append(f)
    mean = rng.randn(10, 1, 128).astype(np.float32)
    std = (rng.rand(10, 1, 128) + 0.5).astype(np.float32)
    sc = str(tmp_path / 'scaler.h5')
    sio.save_arrays(sc, mean=mean, std=std)
    bank = GpuFeatureBank(max_clip_s=60, chunk_len_s=2.0)
    bank.load_feature_scaler(sc)
    bank.add_feature_files(files)
    bank.finalize()
    want = np.concatenate([(sio.load_arrays(f)['feature'] - mean) / std for f in files], axis=1)
    assert np.array_equal(bank.features.cpu().numpy(), want)
    assert tuple(bank[0][0].shape) == (10, bank.chunk_len, 128)

    ys = np.stack([synth_clip(90 + i, 4 * 24000) for i in range(2)])
    ex = BaselineExtractor('melspecgcc', device=DEV)
    bank = GpuFeatureBank(ex, max_clip_s=60, chunk_len_s=2.0)
    bank.add_clips(ys, ['a', 'b'])
    m, s = bank.fit_scaler()
    assert tuple(m.shape) == (10, 1, 128) and bank.n_scaler_channels == 10
    feats = torch.cat(bank.blocks, dim=1).double()
    torch.testing.assert_close(m[:, 0].double(), feats.mean(dim=1), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(s[:, 0].double(), feats.std(dim=1, unbiased=False), rtol=1e-4, atol=1e-5)
    raw = feats.float().clone()
    bank.finalize()
    want = ((raw.cpu() - m.cpu()) / s.cpu()).numpy()
    np.testing.assert_allclose(bank.features.cpu().numpy(), want, rtol=1e-6, atol=1e-6)

    salsa = GpuFeatureBank(SalsaExtractor(), max_clip_s=60, chunk_len_s=2.0)
    salsa.add_clips(ys, ['a', 'b'])
    assert tuple(salsa.fit_scaler()[0].shape) == (4, 1, salsa.blocks[0].shape[-1]) and salsa.n_scaler_channels == 4
