"""The decoder's self-attention stage without a GPU: the float64 reference of tests/attn_reference.py against
torch's nn.MultiheadAttention + nn.LayerNorm, the model's keys, checkpoints and CPU composition, the trainer, the plumbing of the
new keywords, and the launchers' refusals (which are decided before any device call)."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

import attn_reference as ar
from salsa_amd import _lib
from salsa_amd.crnn.model import AttnBlock, Decoder, SeldCRNN

ATTN_SUFFIXES = ('mha.in_proj_weight', 'mha.in_proj_bias', 'mha.out_proj.weight', 'mha.out_proj.bias', 'norm.weight', 'norm.bias')


def _rng(seed):
    return np.random.default_rng(seed)


@pytest.mark.parametrize('B,T,d,heads', [(2, 7, 64, 2), (1, 33, 128, 4), (3, 5, 96, 3)])
def test_float64_reference_agrees_with_torch(B, T, d, heads):
    """forward and every gradient of one block (no dropout) to 1e-10, the packed (B, T, 3, heads, dh) layout against torch's own
    q / k / v split of the in-projection"""
    torch.manual_seed(B * 100 + T)
    mha = nn.MultiheadAttention(d, heads, dropout=0.0, batch_first=True).double()
    norm = nn.LayerNorm(d).double()
    with torch.no_grad():
        mha.in_proj_bias.normal_(0, 0.3)
        mha.out_proj.bias.normal_(0, 0.3)
        norm.weight.uniform_(0.5, 1.5)
        norm.bias.normal_(0, 0.3)
    x = torch.randn(B, T, d, dtype=torch.float64, requires_grad=True)
    y = norm(x + mha(x, x, x)[0])
    gy = torch.randn_like(y)
    y.backward(gy)
    P = {k: v.detach().numpy() for k, v in list(mha.named_parameters()) + [('gamma', norm.weight), ('beta', norm.bias)]}
    xn = x.detach().numpy()
    # forward through the reference's pieces
    qkv = (xn @ P['in_proj_weight'].T + P['in_proj_bias']).reshape(B, T, 3, heads, d // heads)
    a, lse = ar.attn_core_fwd(qkv)
    # torch's own split: q, k, v = chunk(3) of the projection, heads = consecutive blocks of dh
    q, k, v = (t.reshape(B, T, heads, d // heads).transpose(0, 2, 1, 3) for t in np.split(xn @ P['in_proj_weight'].T + P['in_proj_bias'], 3, axis=-1))
    s = q @ k.transpose(0, 1, 3, 2) / np.sqrt(d // heads)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    np.testing.assert_allclose(a, (p @ v).transpose(0, 2, 1, 3).reshape(B, T, d), rtol=0, atol=1e-12)
    np.testing.assert_allclose(lse, np.log(np.exp(s).sum(-1)), rtol=0, atol=1e-12)
    pre = a @ P['out_proj.weight'].T + P['out_proj.bias']
    yn, mean, rstd = ar.add_layernorm_fwd(pre, xn, P['gamma'], P['beta'], norm.eps)
    np.testing.assert_allclose(yn, y.detach().numpy(), rtol=0, atol=1e-10)
    np.testing.assert_allclose(ar.block_fwd(xn, P['in_proj_weight'], P['in_proj_bias'], P['out_proj.weight'], P['out_proj.bias'],
                                            P['gamma'], P['beta'], heads, norm.eps), yn, rtol=0, atol=1e-12)
    # backward through the reference's pieces
    dz, dgamma, dbeta = ar.add_layernorm_bwd(gy.numpy(), pre, xn, P['gamma'], mean, rstd)
    np.testing.assert_allclose(dgamma, norm.weight.grad.numpy(), rtol=0, atol=1e-10)
    np.testing.assert_allclose(dbeta, norm.bias.grad.numpy(), rtol=0, atol=1e-10)
    np.testing.assert_allclose(dz.reshape(-1, d).T @ a.reshape(-1, d), mha.out_proj.weight.grad.numpy(), rtol=0, atol=1e-10)
    np.testing.assert_allclose(dz.reshape(-1, d).sum(0), mha.out_proj.bias.grad.numpy(), rtol=0, atol=1e-10)
    d_qkv = ar.attn_core_bwd(qkv, a, lse, dz @ P['out_proj.weight']).reshape(B * T, 3 * d)
    np.testing.assert_allclose(d_qkv.T @ xn.reshape(-1, d), mha.in_proj_weight.grad.numpy(), rtol=0, atol=1e-10)
    np.testing.assert_allclose(d_qkv.sum(0), mha.in_proj_bias.grad.numpy(), rtol=0, atol=1e-10)
    np.testing.assert_allclose(dz + (d_qkv @ P['in_proj_weight']).reshape(B, T, d), x.grad.numpy(), rtol=0, atol=1e-10)


def test_float32_evaluation_lands_near_and_not_on_the_float64_one():
    """the yardstick of the GPU bounds: the same formulas in float32 are close to float64 and not equal to it"""
    r = _rng(3)
    qkv = r.standard_normal((2, 40, 3, 4, 32)).astype(np.float32)
    g = r.standard_normal((2, 40, 128)).astype(np.float32)
    o64, l64 = ar.attn_core_fwd(qkv)
    o32, l32 = ar.attn_core_fwd(qkv, np.float32)
    assert o32.dtype == np.float32 and l32.dtype == np.float32
    d64, d32 = ar.attn_core_bwd(qkv, o64, l64, g), ar.attn_core_bwd(qkv, o32, l32, g, np.float32)
    for a, b in ((o32, o64), (l32, l64), (d32, d64)):
        err = np.abs(a.astype(np.float64) - b).max()
        assert 0 < err < 1e-4 * max(1.0, np.abs(b).max())
    x, res = r.standard_normal((9, 256)).astype(np.float32), r.standard_normal((9, 256)).astype(np.float32) + 1e3
    gm, bt, dy = (r.standard_normal(s).astype(np.float32) for s in ((256,), (256,), (9, 256)))
    f64, f32 = ar.add_layernorm_fwd(x, res, gm, bt), ar.add_layernorm_fwd(x, res, gm, bt, dtype=np.float32)
    b64, b32 = ar.add_layernorm_bwd(dy, x, res, gm, *f64[1:]), ar.add_layernorm_bwd(dy, x, res, gm, *f32[1:], dtype=np.float32)
    for a, b in zip(f32 + b32, f64 + b64):
        assert a.dtype == np.float32
        err = np.abs(a.astype(np.float64) - b).max()
        assert 0 < err < 1e-3 * max(1.0, np.abs(b).max())


def test_default_model_has_no_attention_key():
    keys = set(SeldCRNN().state_dict())
    assert not any('attn' in k for k in keys)
    assert keys == set(SeldCRNN(n_attn_layers=0).state_dict())
    assert len(SeldCRNN().decoder.attn) == 0


@pytest.mark.parametrize('decoder_type,d', [('bigru', 512), ('gru', 256)])
def test_attention_keys_shapes_and_checkpoint_round_trip(decoder_type, d):
    from salsa_amd.crnn.checkpoint import to_reference_key
    model = SeldCRNN(decoder_type=decoder_type, n_attn_layers=2)
    sd = model.state_dict()
    want = {'decoder.attn.%d.%s' % (i, s) for i in range(2) for s in ATTN_SUFFIXES}
    assert {k for k in sd if 'attn' in k} == want
    assert set(sd) - want == set(SeldCRNN(decoder_type=decoder_type).state_dict())
    for i in range(2):
        pre = 'decoder.attn.%d.' % i
        assert tuple(sd[pre + 'mha.in_proj_weight'].shape) == (3 * d, d) and tuple(sd[pre + 'mha.in_proj_bias'].shape) == (3 * d,)
        assert tuple(sd[pre + 'mha.out_proj.weight'].shape) == (d, d) and tuple(sd[pre + 'mha.out_proj.bias'].shape) == (d,)
        assert tuple(sd[pre + 'norm.weight'].shape) == (d,) and tuple(sd[pre + 'norm.bias'].shape) == (d,)
        assert model.decoder.attn[i].mha.head_dim == d // 8
    assert all(to_reference_key(k) == k for k in want)
    ref_sd = model.reference_state_dict()
    other = SeldCRNN(decoder_type=decoder_type, n_attn_layers=2)
    assert other.load_reference_state_dict(ref_sd) == ([], [])
    for k, v in other.state_dict().items():
        assert torch.equal(v, sd[k]), k
    plain = {k: v for k, v in ref_sd.items() if 'attn' not in k}             # what a reference checkpoint holds
    with pytest.raises(RuntimeError, match='decoder.attn.0.mha.in_proj_weight'):
        other.load_reference_state_dict(plain, strict=True)
    missing, unexpected = other.load_reference_state_dict(plain, strict=False)
    assert set(missing) == want and unexpected == []


@pytest.mark.parametrize('decoder_type', ['bigru', 'gru', 'lstm', 'bilstm'])
def test_cpu_decoder_equals_the_torch_modules_composed_by_hand(decoder_type):
    torch.manual_seed(11)
    dec = Decoder(64, 3, 32, decoder_type, 'avg', n_attn_layers=2, n_attn_heads=4).eval()
    d = 64 if decoder_type.startswith('bi') else 32
    assert all(b.mha.embed_dim == d for b in dec.attn)
    feat = torch.randn(2, 64, 9, 5, requires_grad=True)
    out = dec(feat)
    loss = out['event_frame_logit'].square().sum() + out['doa_frame_output'].sum()
    grads = torch.autograd.grad(loss, [feat] + list(dec.parameters()))
    seq = feat.mean(dim=3).transpose(1, 2)
    seq, _ = dec.rnn(seq)
    for b in dec.attn:
        seq = b.norm(seq + b.drop(b.mha(seq, seq, seq)[0]))
    ev = dec.event(seq)
    doa = torch.cat([torch.tanh(dec.x(seq)), torch.tanh(dec.y(seq)), torch.tanh(dec.z(seq))], dim=-1)
    torch.testing.assert_close(out['event_frame_logit'], ev, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(out['doa_frame_output'], doa, rtol=1e-5, atol=1e-6)
    want = torch.autograd.grad(ev.square().sum() + doa.sum(), [feat] + list(dec.parameters()))
    for g, w in zip(grads, want):
        torch.testing.assert_close(g, w, rtol=1e-4, atol=1e-5 * max(1.0, float(w.abs().max())))


def test_trainer_step_moves_every_attention_parameter():
    from salsa_amd.crnn.train import Trainer, synthetic_batch
    tr = Trainer('cpu', amp_dtype=None, n_attn_layers=2, decoder_size=32, n_attn_heads=4)
    assert tr.n_attn_layers == 2 and tr.n_attn_heads == 4
    named = {k: p for k, p in tr.raw_model.named_parameters() if '.attn.' in k}
    assert len(named) == 12
    before = {k: p.detach().clone() for k, p in named.items()}
    x, sed, doa = synthetic_batch(2, 'cpu', n_frames=64)
    loss = tr.train_step(x, sed, doa)[0]
    assert torch.isfinite(loss)
    for k, p in named.items():
        assert p.grad is not None and float(p.grad.abs().max()) > 0, k
        assert not torch.equal(p.detach(), before[k]), k


def test_dropout_off_covers_the_blocks():
    from salsa_amd.crnn.testing import dropout_off
    dec = Decoder(64, 3, 32, 'bigru', 'avg', n_attn_layers=2, n_attn_heads=4, attn_dropout=0.5).train()
    assert all(isinstance(b.drop, nn.Dropout) and b.drop.p == 0.5 and b.mha.dropout == 0.0 for b in dec.attn)
    feat = torch.randn(2, 64, 9, 5)
    with dropout_off(dec):
        assert all(b.drop.p == 0.0 for b in dec.attn)
        a, b = dec(feat)['event_frame_logit'], dec(feat)['event_frame_logit']
    assert torch.equal(a, b)
    assert all(b.drop.p == 0.5 for b in dec.attn)
    assert not torch.equal(dec(feat)['event_frame_logit'], dec(feat)['event_frame_logit'])


def test_bad_keywords_are_refused():
    with pytest.raises(ValueError, match='heads'):
        SeldCRNN(n_attn_layers=1, n_attn_heads=7)                              # 512 % 7
    with pytest.raises(ValueError, match='heads'):
        Decoder(512, 12, 256, 'gru', 'avg', n_attn_layers=2, n_attn_heads=6)   # 256 % 6
    with pytest.raises(ValueError, match='n_attn_layers'):
        SeldCRNN(n_attn_layers=-1)
    with pytest.raises(ValueError, match='heads'):
        AttnBlock(64, 0)
    with pytest.raises(NotImplementedError):                                   # the refusal this stage does not lift
        SeldCRNN(decoder_type='transformer', n_attn_layers=2)


def test_checkpoints_store_the_stage_and_resume_checks_it(tmp_path):
    from salsa_amd.crnn import fit
    from salsa_amd.crnn.train import Trainer
    tr = Trainer('cpu', amp_dtype=None, n_attn_layers=2, decoder_size=32, n_attn_heads=4)
    loader = types.SimpleNamespace(seed=5)
    path = str(tmp_path / 'epoch=000.ckpt')
    fit._save(path, tr, loader, 0, 1, dict(steps=[]), None)
    ckpt = torch.load(path, map_location='cpu', weights_only=False)
    assert ckpt['n_attn_layers'] == 2 and ckpt['n_attn_heads'] == 4
    assert 'decoder.attn.1.norm.bias' in ckpt['state_dict']
    assert fit._load(path, tr, loader)['epoch'] == 0
    with pytest.raises(ValueError, match='n_attn_layers'):
        fit._load(path, Trainer('cpu', amp_dtype=None, decoder_size=32), loader)
    with pytest.raises(ValueError, match='n_attn_heads'):
        fit._load(path, Trainer('cpu', amp_dtype=None, n_attn_layers=2, decoder_size=32, n_attn_heads=8), loader)
    plain = Trainer('cpu', amp_dtype=None, decoder_size=32)
    fit._save(path, plain, loader, 0, 1, dict(steps=[]), None)
    assert torch.load(path, map_location='cpu', weights_only=False)['n_attn_layers'] == 0
    with pytest.raises(ValueError, match='n_attn_layers'):
        fit._load(path, tr, loader)


NEW_EXPORTS = ('salsa_nn_attn_supported', 'salsa_nn_attn_fwd', 'salsa_nn_attn_bwd', 'salsa_nn_add_layernorm_ws_bytes',
               'salsa_nn_add_layernorm_fwd', 'salsa_nn_add_layernorm_bwd')


def test_exports_build_list_and_switch():
    text = open(os.path.join(_lib.INCLUDE_DIR, 'salsa_nn.h')).read()
    for name in NEW_EXPORTS:
        assert name + '(' in text and name in _lib.NN_EXPORTS
    assert _lib.PROTOTYPES['salsa_nn.h']['salsa_nn_add_layernorm_ws_bytes'][0] is C.c_size_t
    assert os.path.join(_lib.CSRC_DIR, 'attention.hip') in _lib.build_command()
    assert open(os.path.join(_lib.CSRC_DIR, 'attention.hip')).read().split('\n#include')[1].strip() == '"build_guard.h"'
    from salsa_amd.crnn import attention
    assert attention.HIP_ATTN is True or os.environ.get('SALSA_HIP_ATTN') == '0'
    assert 'SALSA_HIP_ATTN' in open(os.path.join(os.path.dirname(_lib.INCLUDE_DIR), 'README.md')).read()


def test_launchers_refuse_before_any_device_call():
    L = _lib.load()
    assert [L.salsa_nn_attn_supported(T, 8, dh) for T, dh in ((1, 64), (512, 32), (0, 64), (513, 64), (40, 48), (40, 128))] == [1, 1, 0, 0, 0, 0]
    assert L.salsa_nn_attn_supported(40, 0, 64) == 0
    buf = np.zeros(64, np.float32)
    p = C.c_void_p(buf.ctypes.data)                                            # a HOST pointer: a launch with it would be an error
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert L.salsa_nn_attn_fwd(*args, 1, 40, 8, 64, None) == -1
    for T, heads, dh in ((0, 8, 64), (513, 8, 64), (40, 8, 48), (40, 0, 64), (-1, 8, 32)):
        assert L.salsa_nn_attn_fwd(p, p, p, 1, T, heads, dh, None) == -1
        assert L.salsa_nn_attn_bwd(p, p, p, p, p, 1, T, heads, dh, None) == -1
    assert L.salsa_nn_attn_fwd(p, p, p, 0, 40, 8, 64, None) == -1
    for hole in range(5):
        args = [p] * 5
        args[hole] = None
        assert L.salsa_nn_attn_bwd(*args, 1, 40, 8, 64, None) == -1
    assert L.salsa_nn_add_layernorm_ws_bytes(0, 256) == 0 and L.salsa_nn_add_layernorm_ws_bytes(5, 300) == 0
    assert L.salsa_nn_add_layernorm_ws_bytes(7, 256) == 2 * 2 * 256 * 4        # two workgroups of four rows
    assert L.salsa_nn_add_layernorm_ws_bytes(9600, 512) == L.salsa_nn_add_layernorm_ws_bytes(1 << 20, 512) == 256 * 2 * 512 * 4
    for hole in range(7):
        args = [p] * 7
        args[hole] = None
        assert L.salsa_nn_add_layernorm_fwd(*args, 4, 256, 1e-5, None) == -1
    for M, Cn in ((0, 256), (4, 128), (4, 384), (-3, 512)):
        assert L.salsa_nn_add_layernorm_fwd(*([p] * 7), M, Cn, 1e-5, None) == -1
        assert L.salsa_nn_add_layernorm_bwd(*([p] * 10), 1 << 20, M, Cn, None) == -1
    for hole in range(10):
        args = [p] * 10
        args[hole] = None
        assert L.salsa_nn_add_layernorm_bwd(*args, 1 << 20, 4, 256, None) == -1
    assert L.salsa_nn_add_layernorm_bwd(*([p] * 10), 16, 4, 256, None) == -5   # a workspace too small
