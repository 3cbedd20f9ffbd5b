"""GPU tests of the ACCDOA output format: salsa_nn_accdoa_loss against a float64 restatement of the reference's loss and against
fixture g25, salsa_nn_accdoa_sed bit-equal to numpy's float32 expression, bf16 training with output_format 'accdoa' (the event head
stays bit-identical, in both head paths), the fused loss against the torch path, the default trainer's loss kernel, and
inference through infer_pipelined."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def loss64(p, m, t):
    """float64 restatement of compute_classwise_accdoa_loss (models/interfaces.py:284-302): the doa loss and d loss / d p"""
    p, m, t = (np.asarray(a, dtype=np.float64) for a in (p, m, t))
    nc = m.shape[-1]
    rows = m.size // nc
    e = p - t
    sq = e ** 2
    loss = float(np.sum((sq[..., :nc] + sq[..., nc:2 * nc] + sq[..., 2 * nc:]) * m) / rows)
    return loss, 2.0 * e * np.concatenate([m, m, m], axis=-1) / rows


def inputs(shape, seed, mask='random'):
    B, T, nc = shape
    g = torch.Generator().manual_seed(seed)
    p = torch.tanh(torch.randn(B, T, 3 * nc, generator=g))
    m = (torch.rand(B, T, nc, generator=g) < 0.3).float()
    if mask == 'off':
        m.zero_()
    elif mask == 'on':
        m.fill_(1.0)
    v = torch.randn(B, T, 3, nc, generator=g)
    t = (v / v.norm(dim=2, keepdim=True) * m[:, :, None, :]).reshape(B, T, 3 * nc)
    return p, m, t


def kernel(p, m, t, g_logit=True):
    """one salsa_nn_accdoa_loss call -> (out3, g_logit or None, g_doa) on the host; g_logit starts as NaN to show the fill"""
    from salsa_amd import _lib
    p, m, t = (a.to(DEV).contiguous() for a in (p, m, t))
    nc = m.shape[-1]
    out = torch.full((3,), float('nan'), device=DEV)
    ws = torch.empty(64, dtype=torch.float64, device=DEV)
    gl = torch.full(m.shape, float('nan'), device=DEV) if g_logit else None
    gd = torch.full(p.shape, float('nan'), device=DEV)
    ptr = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None          # noqa: E731
    rc = _lib.load().salsa_nn_accdoa_loss(ptr(p), ptr(m), ptr(t), m.numel() // nc, nc, ptr(out), ptr(gl), ptr(gd), ptr(ws),
                                          C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu(), None if gl is None else gl.cpu(), gd.cpu()


@pytest.mark.parametrize('shape,mask', [((32, 80, 12), 'random'), ((3, 37, 14), 'random'), ((1, 1, 12), 'random'),
                                        ((1, 1, 1), 'on'), ((5, 17, 14), 'off'), ((32, 80, 12), 'on'), ((7, 3, 1), 'random')])
def test_accdoa_loss_kernel_against_float64(shape, mask):
    p, m, t = inputs(shape, sum(shape), mask)
    ref, gref = loss64(p.numpy(), m.numpy(), t.numpy())
    out, gl, gd = kernel(p, m, t)
    err = abs(float(out[0]) - ref)
    bound = 1e-6 * abs(ref) + 1e-30
    gerr, gbound = float(np.abs(gd.numpy() - gref).max()), 5e-7 * float(np.abs(gref).max()) + 1e-30
    print('accdoa loss %s mask %s: loss err %.3g / bound %.3g, grad err %.3g / bound %.3g' % (shape, mask, err, bound, gerr, gbound))
    assert err <= bound and gerr <= gbound
    assert float(out[2]) == float(out[0]) and float(out[1]) == 0.0
    assert torch.count_nonzero(gl) == 0 and not torch.isnan(gl).any()
    if mask == 'off':
        assert float(out[0]) == 0.0 and torch.count_nonzero(gd) == 0
    out2, gl2, gd2 = kernel(p, m, t)
    assert torch.equal(out, out2) and torch.equal(gd, gd2) and torch.equal(gl, gl2)     # fixed-order sums: bit-reproducible
    out3, none, gd3 = kernel(p, m, t, g_logit=False)                                 # no logit buffer: nothing else changes
    assert none is None and torch.equal(out3, out) and torch.equal(gd3, gd)


@pytest.mark.parametrize('i', [0, 1])
def test_fused_loss_on_the_fixture(i):
    """the autograd Function (salsa_nn_accdoa_loss + salsa_nn_seld_loss_bwd) on g25 (a)'s inputs, with a scaled upstream gradient"""
    from salsa_amd.crnn import loss as L
    meta, a = load_golden('g25_accdoa')
    shape = tuple(meta['loss_shapes'][i])
    B, T, nc = shape
    g = torch.Generator().manual_seed(meta['loss_seed'])
    p = torch.tanh(torch.randn(B, T, 3 * nc, generator=g))
    m = (torch.rand(B, T, nc, generator=g) < 0.3).float()
    v = torch.randn(B, T, 3, nc, generator=g)
    t = (v / v.norm(dim=2, keepdim=True) * m[:, :, None, :]).reshape(B, T, 3 * nc)
    assert L.FUSED_LOSS
    p = p.to(DEV).requires_grad_(True)
    logit = torch.randn(shape, device=DEV, requires_grad=True)
    loss, sed_l, doa_l = L.accdoa_loss({'event_frame_logit': logit, 'doa_frame_output': p}, m.to(DEV), t.to(DEV))
    assert loss.grad_fn is not None and type(loss.grad_fn).__name__.startswith('_AccdoaLoss')
    key = 'loss:%dx%dx%d' % shape
    np.testing.assert_allclose(loss.item(), a[key + ':loss'][0], rtol=2e-6)
    (loss * 1.5 + doa_l * 0.25).backward()
    ref = 1.75 * a[key + ':grad']
    err = float(np.abs(p.grad.cpu().numpy() - ref).max())
    print('g25 %s: grad err %.3g / bound %.3g' % (shape, err, 1e-6 * np.abs(ref).max()))
    assert err <= 1e-6 * np.abs(ref).max()
    assert torch.count_nonzero(logit.grad) == 0


@pytest.mark.parametrize('shape', [(32, 600, 12), (3, 37, 14), (1, 1, 1)])
def test_accdoa_sed_is_bit_equal_to_numpy(shape):
    from salsa_amd.crnn.nn_ops import accdoa_sed
    from salsa_amd.crnn.postprocess import sed_from_accdoa
    B, T, nc = shape
    g = torch.Generator().manual_seed(B * T + nc)
    y = torch.randn(B, T, 3 * nc, generator=g) * torch.exp(torch.randn(B, T, 1, generator=g) * 3)   # lengths over decades
    y[..., :nc][torch.rand(B, T, nc, generator=g) < 0.1] = 0.0
    y = y.numpy().astype(np.float32)
    got = accdoa_sed(torch.from_numpy(y).to(DEV), nc).cpu().numpy()
    ref = sed_from_accdoa(y, nc)
    n_diff = int((got != ref).sum())
    print('accdoa sed %s: %d of %d differ' % (shape, n_diff, ref.size))
    assert got.shape == ref.shape and n_diff == 0


def _train(steps, **kw):
    from salsa_amd.crnn.train import Trainer, synthetic_batch
    tr = Trainer(DEV, total_steps=10 ** 6, output_format='accdoa', **kw)
    x, sed, doa = synthetic_batch(8, DEV, seed=3)
    init = {k: p.detach().clone() for k, p in tr.raw_model.named_parameters()}
    losses = [float(tr.train_step(x, sed, doa)[0]) for _ in range(steps)]
    return tr, init, losses


@pytest.mark.parametrize('batched', [True, False])
def test_bf16_training_keeps_the_event_head(batched, monkeypatch):
    from salsa_amd.crnn import model
    monkeypatch.setattr(model, 'BATCHED_HEADS', batched)
    tr, init, losses = _train(10)
    print('accdoa bf16 training, batched heads %s: loss %s' % (batched, ['%.4f' % v for v in losses]))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    moved = {}
    for k, p in tr.raw_model.named_parameters():
        if k.startswith('decoder.event.'):
            assert p.grad is not None and torch.count_nonzero(p.grad) == 0, k
            assert torch.equal(p.detach(), init[k]), k
        else:
            moved[k] = not torch.equal(p.detach(), init[k])
    for prefix in ('decoder.x.', 'decoder.y.', 'decoder.z.', 'decoder.gru.', 'encoder.'):
        group = [v for k, v in moved.items() if k.startswith(prefix)]
        assert group and all(group), (prefix, [k for k, v in moved.items() if k.startswith(prefix) and not v])


def test_fused_loss_agrees_with_the_torch_path(monkeypatch):
    """one bf16 step each (same seed, same batch): the loss and the x-head gradient of the fused loss and of the torch path"""
    from salsa_amd.crnn import loss as L
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(L, 'FUSED_LOSS', fused)
        tr, _, losses = _train(1)
        res[fused] = (losses[0], tr.raw_model.decoder.x.fc2.weight.grad.clone(), tr.raw_model.decoder.gru.weight_hh_l1.grad.clone())
        del tr
    dl = abs(res[True][0] - res[False][0])
    print('fused vs torch accdoa loss: %.8g vs %.8g (diff %.3g)' % (res[True][0], res[False][0], dl))
    assert dl <= 1e-5 * abs(res[False][0])
    for a, b in zip(res[True][1:], res[False][1:]):
        err, scale = float((a - b).abs().max()), float(b.abs().max())
        print('  grad err %.3g / bound %.3g' % (err, 1e-3 * scale))
        assert err <= 1e-3 * scale


def test_default_trainer_keeps_the_reg_xyz_loss_kernel(monkeypatch):
    from salsa_amd import _lib
    from salsa_amd.crnn.train import Trainer, synthetic_batch
    L = _lib.load()
    calls = {'salsa_nn_seld_loss': 0, 'salsa_nn_accdoa_loss': 0}
    for name in calls:
        real = getattr(L, name)

        def counted(*a, _real=real, _name=name):
            calls[_name] += 1
            return _real(*a)
        monkeypatch.setattr(L, name, counted)
    x, sed, doa = synthetic_batch(4, DEV, seed=2)
    tr = Trainer(DEV, total_steps=10 ** 6)
    assert tr.output_format == 'reg_xyz'
    tr.train_step(x, sed, doa)
    assert calls == {'salsa_nn_seld_loss': 1, 'salsa_nn_accdoa_loss': 0}
    prob, _ = tr.infer(x)
    assert float(prob.min()) >= 0.0 and float(prob.max()) <= 1.0              # sigmoid probabilities
    tr = Trainer(DEV, total_steps=10 ** 6, output_format='accdoa')
    tr.train_step(x, sed, doa)
    assert calls == {'salsa_nn_seld_loss': 1, 'salsa_nn_accdoa_loss': 1}


def test_infer_pipelined_with_accdoa():
    from salsa_amd.crnn.infer import infer_pipelined
    from salsa_amd.crnn.postprocess import sed_from_accdoa, to_dcase_rows
    from salsa_amd.crnn.train import Trainer
    tr, _, _ = _train(3)
    g = torch.Generator(device='cpu').manual_seed(9)
    feats = torch.randn(6, 7, 640, 200, generator=g).to(DEV)
    with torch.no_grad():
        thr = float(torch.quantile(tr.infer(feats[:2])[0].flatten(), 0.9))     # a threshold that some classes pass
    seen = []

    def forward(x):
        prob, xyz = tr.infer(x)
        seen.append((prob.cpu().numpy(), xyz.cpu().numpy()))
        return prob, xyz
    rows = infer_pipelined(6, lambda lo, hi: feats[lo:hi], forward, sub_batch=4, depth=2, sed_threshold=thr, n_label_frames=80)
    prob = np.concatenate([s[0] for s in seen])
    xyz = np.concatenate([s[1] for s in seen])
    assert np.array_equal(prob, sed_from_accdoa(xyz, 12))
    n = 0
    for i in range(6):
        want = to_dcase_rows(sed_from_accdoa(xyz[i], 12), xyz[i], sed_threshold=thr, max_nframes_per_file=80)
        assert rows[i] == want, i
        n += len(want)
    print('infer_pipelined accdoa: %d rows over 6 clips (threshold %.4g)' % (n, thr))
    assert isinstance(tr, Trainer) and n > 0
