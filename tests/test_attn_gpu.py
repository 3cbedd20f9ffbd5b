"""The decoder's self-attention stage on the GPU: the attention core (salsa_nn_attn_fwd / _bwd) and the fused
residual add + LayerNorm (salsa_nn_add_layernorm_fwd / _bwd) through the C ABI against the float64 reference of
tests/attn_reference.py, their structural properties, the block and decoder against the torch-operator path, and the whole model.

Bound of every comparison with float64: the kernel's maximum error may be at most 4 times the maximum error of the FLOAT32
evaluation of the same reference on that case, plus one float32 ulp of the tensor's largest magnitude.  (4: another summation order,
and the device's exp / log / sqrt against numpy's.)  Measured ratios kernel error / float32-reference error are in MEASURED below."""
import ctypes as C

import numpy as np
import pytest
import torch

import attn_reference as ar
from salsa_amd import _lib

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARD = 1024
FACTOR = 4.0
MEASURED = """largest ratio (kernel error) / (float32-reference error) over every case of a family, per tensor, on one MI355X
(0.00: the kernel's error was zero; the attention yardstick is the largest error of four float32 evaluations, _float32_evaluations):
  family      out           lse           d_q           d_k           d_v
  gauss1      2.63 (T 2)    2.28 (T 2)    1.63          1.74          1.50
  gauss8      3.02 (T 31)   3.25 (T 33)   2.56          1.98          1.72
  dominant    0.00          2.74          0.00          0.00          2.16
  equal_keys  1.92          2.32          1.14          2.23          2.06
  offset      1.32          1.00          3.39 (T 2)    3.15 (T 2)    1.11
  zero_dout   2.04          2.50 (T 1)    1.51          1.87          2.10
  (no family needed more than 4.  The largest ratios sit at T <= 33 with two heads, where both errors are the maximum of a few
  roundings; at T >= 127 every ratio was below 2.3.  'dominant': dS = P o dO (V - O)^T is exactly zero where one key holds the row.)
  add + LayerNorm   y     mean   rstd   dx     dgamma  dbeta
  gauss             1.27  4.86*  1.06   1.28   1.00    0.99
  constant          0.00  0.50   1.00   1.63   0.00    0.86
  offset (1e3)      1.00  1.00   1.03   1.00   1.00    1.21
  (* M = 1, C = 256: one row's mean, error 2.5e-8 against a yardstick of 5e-9 -- both below the one-ulp floor of the tensor, which
  is what admits it; from M = 7 on the ratio was at most 1.2.)
  decoder (outputs and every parameter gradient, HIP blocks against the torch-operator leg): at most 2.19 (bigru), 1.86 (gru)."""


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _guarded(shape):
    """a NaN-filled buffer with the tensor in its middle -> (buffer, view)"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float('nan'), dtype=torch.float32, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _check_guards(*bufs):
    for buf, view in bufs:
        assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + view.numel():]).all()), 'a guard band was written'
        assert not bool(torch.isnan(view).any()), 'an output element was not written'


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _holds(name, got, ref64, ref32, case):
    """ref32: one float32 evaluation, or a list of them (the yardstick is then their largest error)"""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref64).max()
    yard = max(np.abs(r.astype(np.float64) - ref64).max() for r in (ref32 if isinstance(ref32, list) else [ref32]))
    floor = float(np.spacing(np.float32(np.abs(ref64).max())))
    print('RATIO %s %s err %.3e yard %.3e floor %.3e ratio %s' % (case, name, err, yard, floor, '%.2f' % (err / yard) if yard > 0 else '-'))
    assert np.isfinite(got).all(), (case, name)
    assert err <= FACTOR * yard + floor, '%s %s: error %.3e > %g x %.3e + %.3e' % (case, name, err, FACTOR, yard, floor)


# ---- attention core ---------------------------------------------------------------------------------------------------------------
FAMILIES = ('gauss1', 'gauss8', 'dominant', 'equal_keys', 'offset', 'zero_dout')


def _attn_case(family, B, T, H, dh, seed):
    r = np.random.default_rng(seed)
    qkv = r.standard_normal((B, T, 3, H, dh))
    d_out = r.standard_normal((B, T, H * dh))
    if family == 'gauss8':
        qkv[:, :, 0] *= 8.0                                                    # logits of standard deviation ~ 8
    elif family == 'dominant':                                                 # one key per (sample, head) beats the others by > 100
        u = np.ones(dh) / np.sqrt(dh)
        qkv[:, :, 0] = 6.0 * u + 0.3 * qkv[:, :, 0]
        qkv[:, :, 1] *= 0.3
        for b in range(B):
            for h in range(H):
                qkv[b, (3 * h + b) % T, 1, h] = 25.0 * np.sqrt(dh) * u
    elif family == 'equal_keys':                                               # uniform 1 / T rows
        qkv[:, :, 1] = qkv[:, :1, 1]
    elif family == 'offset':                                                   # + 1e3 on the logits of one row, through q
        qkv[:, :, 1, :, -1] = 1.0
        qkv[:, T // 2, 0, :, -1] += 1e3 * np.sqrt(dh)
    elif family == 'zero_dout':
        d_out[:, ::2] = 0.0
        if B > 1:
            d_out[-1] = 0.0
    qkv, d_out = qkv.astype(np.float32), d_out.astype(np.float32)
    if family == 'dominant' and T > 1:
        s = np.einsum('bihd,bjhd->bhij', qkv[:, :, 0].astype(np.float64), qkv[:, :, 1].astype(np.float64)) / np.sqrt(dh)
        top2 = np.sort(s, axis=-1)[..., -2:]
        assert (top2[..., 1] - top2[..., 0]).min() > 100
    return qkv, d_out


def _run_core(qkv, d_out):
    """the C ABI on numpy inputs, every output inside NaN guard bands -> out, lse, d_qkv (numpy)"""
    L = _lib.load()
    B, T, _, H, dh = qkv.shape
    tq, tg = torch.from_numpy(qkv).to(DEV), torch.from_numpy(d_out).to(DEV)
    out, lse, dq = _guarded((B, T, H * dh)), _guarded((B, H, T)), _guarded(qkv.shape)
    assert L.salsa_nn_attn_supported(T, H, dh) == 1
    assert L.salsa_nn_attn_fwd(_ptr(tq), _ptr(out[1]), _ptr(lse[1]), B, T, H, dh, _stream()) == 0
    assert L.salsa_nn_attn_bwd(_ptr(tq), _ptr(out[1]), _ptr(lse[1]), _ptr(tg), _ptr(dq[1]), B, T, H, dh, _stream()) == 0
    torch.cuda.synchronize()
    _check_guards(out, lse, dq)
    return out[1].cpu().numpy(), lse[1].cpu().numpy(), dq[1].cpu().numpy()


def _float32_evaluations(qkv, d_out):
    """The float32 evaluation of the reference under four orders of the head dimension (as it stands, reversed, even then odd, one
    seeded shuffle) -> [(out, lse, d_qkv)], results in the natural order.  The formulas do not fix the order of the sums over the
    head dimension and a float32 result depends on it; on the small cases (T <= 2, two heads, the 'offset' row) the error of ONE
    order is the maximum of two to four roundings, and the ratio of two such maxima exceeds any factor now and then (measured with
    the natural order alone: up to 4.9 at T = 2, 1.0 - 2.5 from T = 31 on), so the yardstick is the largest error of the four."""
    B, T, _, H, dh = qkv.shape
    perms = [np.arange(dh), np.arange(dh)[::-1], np.r_[np.arange(0, dh, 2), np.arange(1, dh, 2)], np.random.default_rng(dh).permutation(dh)]
    evals = []
    for perm in perms:
        inv = np.argsort(perm)
        qp, gp = np.ascontiguousarray(qkv[..., perm]), np.ascontiguousarray(d_out.reshape(B, T, H, dh)[..., perm]).reshape(B, T, H * dh)
        o, l = ar.attn_core_fwd(qp, np.float32)
        g = ar.attn_core_bwd(qp, o, l, gp, np.float32)
        evals.append((o.reshape(B, T, H, dh)[..., inv].reshape(B, T, H * dh), l, g[..., inv]))
    return evals


def _check_core(B, T, H, dh, families=FAMILIES):
    for n, family in enumerate(families):
        qkv, d_out = _attn_case(family, B, T, H, dh, seed=1000 * T + 10 * dh + n)
        out, lse, d_qkv = _run_core(qkv, d_out)
        o64, l64 = ar.attn_core_fwd(qkv)
        g64 = ar.attn_core_bwd(qkv, o64, l64, d_out)
        f32 = _float32_evaluations(qkv, d_out)
        case = '%s B%d T%d H%d dh%d' % (family, B, T, H, dh)
        _holds('out', out, o64, [e[0] for e in f32], case)
        _holds('lse', lse, l64, [e[1] for e in f32], case)
        for i, name in enumerate(('d_q', 'd_k', 'd_v')):
            _holds(name, d_qkv[:, :, i], g64[:, :, i], [e[2][:, :, i] for e in f32], case)
        if family == 'equal_keys':
            np.testing.assert_allclose(lse, np.log(T) + (qkv[:, :, 0].astype(np.float64) * qkv[:, :1, 1]).sum(-1).transpose(0, 2, 1)
                                       / np.sqrt(dh), rtol=0, atol=1e-4 * max(1.0, np.abs(l64).max()))
        if family == 'zero_dout':
            assert not d_qkv[:, ::2, 0].any() and (B == 1 or not d_qkv[-1].any())   # zero d_out rows: exactly zero d_q; a zero sample


# every edge of the kernels' 64-row tiles is in the list (63, 64, 65, 127, 128, 129, ...)
SWEEP_T = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 511, 512)


@pytest.mark.parametrize('dh', [64, 32])
@pytest.mark.parametrize('T', SWEEP_T)
def test_attention_core_time_sweep(T, dh):
    _check_core(1, T, 2, dh)


@pytest.mark.parametrize('B,T,H,dh', [(3, 33, 8, 64), (2, 40, 8, 64), (2, 300, 8, 64), (2, 40, 8, 32)])
def test_attention_core_whole_shapes(B, T, H, dh):
    _check_core(B, T, H, dh)


@pytest.mark.parametrize('T,dh', [(40, 64), (300, 64), (129, 32)])
def test_attention_core_is_bit_repeatable_and_batch_invariant(T, dh):
    qkv, d_out = _attn_case('gauss1', 3, T, 8, dh, seed=5)
    first, again = _run_core(qkv, d_out), _run_core(qkv, d_out)
    alone = _run_core(qkv[1:2], d_out[1:2])
    for a, b, c in zip(first, again, alone):
        assert np.array_equal(a, b)
        assert np.array_equal(a[1:2], c)


# ---- add + LayerNorm --------------------------------------------------------------------------------------------------------------
def _run_ln(x, res, gamma, beta, dy, eps):
    L = _lib.load()
    M, Cn = x.shape
    tx, tr, tg, tb, td = (torch.from_numpy(a).to(DEV) for a in (x, res, gamma, beta, dy))
    y, mean, rstd, dx, dgm, dbt = (_guarded(s) for s in ((M, Cn), (M,), (M,), (M, Cn), (Cn,), (Cn,)))
    ws_bytes = L.salsa_nn_add_layernorm_ws_bytes(M, Cn)
    assert ws_bytes > 0 and ws_bytes % 4 == 0
    ws = _guarded((ws_bytes // 4,))
    assert L.salsa_nn_add_layernorm_fwd(_ptr(tx), _ptr(tr), _ptr(tg), _ptr(tb), _ptr(y[1]), _ptr(mean[1]), _ptr(rstd[1]), M, Cn, eps,
                                        _stream()) == 0
    assert L.salsa_nn_add_layernorm_bwd(_ptr(td), _ptr(tx), _ptr(tr), _ptr(tg), _ptr(mean[1]), _ptr(rstd[1]), _ptr(dx[1]), _ptr(dgm[1]),
                                        _ptr(dbt[1]), _ptr(ws[1]), ws_bytes, M, Cn, _stream()) == 0
    torch.cuda.synchronize()
    _check_guards(y, mean, rstd, dx, dgm, dbt, ws)
    return tuple(t[1].cpu().numpy() for t in (y, mean, rstd, dx, dgm, dbt))


@pytest.mark.parametrize('Cn', [256, 512])
@pytest.mark.parametrize('M', [1, 7, 63, 64, 65, 1280, 9600])
def test_add_layernorm_against_float64(M, Cn):
    """dgamma / dbeta: bit-equal between two runs.  Between two orders of the rows they are NOT promised equal (the partial sums follow
    the row order), and that is not asserted."""
    eps = float(np.float32(1e-5))
    for n, family in enumerate(('gauss', 'constant', 'offset')):
        r = np.random.default_rng(100 * M + Cn + n)
        x, res = r.standard_normal((M, Cn)), r.standard_normal((M, Cn))
        if family == 'constant':                                               # zero variance: rstd = 1 / sqrt(eps)
            x[:], res[:] = r.standard_normal((M, 1)), r.standard_normal((M, 1))
        elif family == 'offset':                                               # the cancellation case of E[z^2] - E[z]^2
            res[:] = 1e3
        gamma, beta, dy = 1.0 + 0.3 * r.standard_normal(Cn), r.standard_normal(Cn), r.standard_normal((M, Cn))
        x, res, gamma, beta, dy = (a.astype(np.float32) for a in (x, res, gamma, beta, dy))
        got = _run_ln(x, res, gamma, beta, dy, eps)
        f64 = ar.add_layernorm_fwd(x, res, gamma, beta, eps)
        f32 = ar.add_layernorm_fwd(x, res, gamma, beta, eps, np.float32)
        b64 = ar.add_layernorm_bwd(dy, x, res, gamma, f64[1], f64[2])
        b32 = ar.add_layernorm_bwd(dy, x, res, gamma, f32[1], f32[2], np.float32)
        case = 'ln-%s M%d C%d' % (family, M, Cn)
        for name, g, a, b in zip(('y', 'mean', 'rstd', 'dx', 'dgamma', 'dbeta'), got, f64 + b64, f32 + b32):
            _holds(name, g, a, b, case)
        if family == 'constant':
            np.testing.assert_allclose(got[2], 1.0 / np.sqrt(eps), rtol=1e-6)
            np.testing.assert_allclose(got[0], np.broadcast_to(beta, (M, Cn)), rtol=0, atol=0)
        again = _run_ln(x, res, gamma, beta, dy, eps)
        for a, b in zip(got, again):
            assert np.array_equal(a, b)


# ---- block and decoder ------------------------------------------------------------------------------------------------------------
_DECODER_REF = {}


def _decoder_case(decoder_type, Tp):
    """the decoder's input, loss weights, parameters and the float64 composition on the CPU (computed once per case)"""
    key = (decoder_type, Tp)
    if key not in _DECODER_REF:
        from salsa_amd.crnn.model import Decoder
        from salsa_amd.crnn.testing import seeded_fill
        g = torch.Generator().manual_seed(7 + Tp)
        dec = Decoder(512, 12, 256, decoder_type, 'avg', n_attn_layers=2)
        seeded_fill(dec, 3)
        feat = torch.randn(3, 512, Tp, 12, generator=g).to(torch.bfloat16)
        w = (torch.randn(3, Tp, 12, generator=g), torch.randn(3, Tp, 36, generator=g))
        ref = Decoder(512, 12, 256, decoder_type, 'avg', n_attn_layers=2).double()
        ref.load_state_dict({k: v.double() for k, v in dec.state_dict().items()})
        ref.eval()
        out = ref(feat.double())
        loss = (out['event_frame_logit'] * w[0].double()).sum() + (out['doa_frame_output'] * w[1].double()).sum()
        grads = torch.autograd.grad(loss, list(ref.parameters()))
        want = {'event': out['event_frame_logit'].detach().numpy(), 'doa': out['doa_frame_output'].detach().numpy()}
        want.update({k: g.numpy() for (k, _), g in zip(ref.named_parameters(), grads)})
        _DECODER_REF[key] = (dec.state_dict(), feat, w, want)
    return _DECODER_REF[key]


@pytest.mark.parametrize('Tp', [40, 300])
@pytest.mark.parametrize('decoder_type', ['bigru', 'gru'])
def test_decoder_hip_blocks_against_the_torch_path(decoder_type, Tp, monkeypatch):
    """Decoder(512, 12, 256, ., 'avg', n_attn_layers=2) in training mode under dropout_off, batch 3: the HIP blocks against the same
    decoder with SALSA_HIP_ATTN=0, both held to the float64 composition by the 4 x rule (the torch-path leg is the float32
    yardstick); with the switch at 1 neither nn.MultiheadAttention.forward nor F.layer_norm is reached."""
    import torch.nn.functional as F
    from salsa_amd.crnn import attention
    from salsa_amd.crnn.model import Decoder
    from salsa_amd.crnn.testing import dropout_off
    sd, feat, w, want = _decoder_case(decoder_type, Tp)
    dec = Decoder(512, 12, 256, decoder_type, 'avg', n_attn_layers=2)
    dec.load_state_dict(sd)
    dec = dec.to(DEV).train()
    x = feat.to(DEV).contiguous(memory_format=torch.channels_last)
    w = [t.to(DEV) for t in w]
    real_mha, real_ln = torch.nn.MultiheadAttention.forward, F.layer_norm

    def leg(hip):
        monkeypatch.setattr(attention, 'HIP_ATTN', hip)
        if hip:
            def refuse(*a, **k):
                raise AssertionError('the torch operator was reached with SALSA_HIP_ATTN=1')
            monkeypatch.setattr(torch.nn.MultiheadAttention, 'forward', refuse)
            monkeypatch.setattr(F, 'layer_norm', refuse)
        else:
            monkeypatch.setattr(torch.nn.MultiheadAttention, 'forward', real_mha)
            monkeypatch.setattr(F, 'layer_norm', real_ln)
        with dropout_off(dec):
            out = dec(x)
            loss = (out['event_frame_logit'] * w[0]).sum() + (out['doa_frame_output'] * w[1]).sum()
            grads = torch.autograd.grad(loss, list(dec.parameters()))
        got = {'event': out['event_frame_logit'].detach().cpu().numpy(), 'doa': out['doa_frame_output'].detach().cpu().numpy()}
        got.update({k: g.cpu().numpy() for (k, _), g in zip(dec.named_parameters(), grads)})
        return got

    hip, ref32 = leg(True), leg(False)
    for k in want:
        _holds(k, hip[k], want[k], ref32[k], 'decoder-%s T%d' % (decoder_type, Tp))


# ---- whole model ------------------------------------------------------------------------------------------------------------------
def test_trainer_bf16_steps_with_blocks_are_finite_move_and_repeat():
    from salsa_amd.crnn.train import Trainer, synthetic_batch
    x, sed, doa = synthetic_batch(4, DEV, seed=2, n_frames=128)
    runs = []
    for _ in range(2):
        tr = Trainer(DEV, total_steps=100, n_attn_layers=2)
        named = {k: p for k, p in tr.raw_model.named_parameters() if '.attn.' in k}
        before = {k: p.detach().clone() for k, p in named.items()}
        losses = [tr.train_step(x, sed, doa)[0] for _ in range(3)]
        runs.append(torch.stack(losses).cpu().numpy())
        assert len(named) == 12 and np.isfinite(runs[-1]).all()
        for k, p in named.items():
            assert not torch.equal(p.detach(), before[k]), k
    assert runs[0].tobytes() == runs[1].tobytes(), runs


def test_trainer_infer_on_long_clips_with_blocks():
    from salsa_amd.crnn.train import Trainer
    tr = Trainer(DEV, n_attn_layers=2)
    x = torch.randn(2, 7, 4800, 200, generator=torch.Generator().manual_seed(1)).to(DEV)
    p, d = tr.infer(x)
    assert p.shape == (2, 600, 12) and d.shape == (2, 600, 36)
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(d).all())


def test_multi_accdoa_step_with_blocks():
    import multi_accdoa_reference as mref
    from salsa_amd.crnn.train import Trainer, synthetic_batch
    tr = Trainer(DEV, total_steps=100, n_attn_layers=2, output_format='multi_accdoa')
    x, _, _ = synthetic_batch(4, DEV, seed=3, n_frames=128)
    _, sed, gt = mref.build_adpit_inputs(4 * 16, 12, seed=5, prefix_only=True)
    sed, gt = (torch.from_numpy(a).to(DEV).reshape(4, 16, -1) for a in (sed, gt))
    loss = tr.train_step(x, sed, gt)[0]
    assert bool(torch.isfinite(loss))
    p, d = tr.infer(x)
    assert p.shape == (4, 16, 36) and d.shape == (4, 16, 108) and bool(torch.isfinite(d).all())
