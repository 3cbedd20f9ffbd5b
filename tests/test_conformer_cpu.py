"""The decoder's Conformer blocks without a GPU: the float64 references of tests/conformer_reference.py against
torch's own modules and against finite differences, the restated dropout mask, the model's keys, checkpoints and CPU composition, the
trainer, the plumbing of the new keywords, and the launchers' refusals (which are decided before any device call)."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import conformer_reference as cr
from salsa_amd import _lib
from salsa_amd.crnn.model import Decoder, SeldCRNN

SUFFIXES = tuple('%s.%s' % (m, s) for m in ('norm_ff1', 'ff1_w1', 'ff1_w2', 'norm_att', 'mha.out_proj', 'norm_conv', 'conv_p1', 'conv_dw',
                                             'conv_norm', 'conv_p2', 'norm_ff2', 'ff2_w1', 'ff2_w2', 'norm_out')
                 for s in ('weight', 'bias')) + ('mha.in_proj_weight', 'mha.in_proj_bias')
RTOL = 1e-9


def _close(got, want, what=''):
    want = np.asarray(want)
    assert np.abs(np.asarray(got) - want).max() <= RTOL * max(1.0, np.abs(want).max()), what


def _block(d=16, heads=2, ff=24, kernel=5, dropout=0.1, seed=0):
    from salsa_amd.crnn.model import ConformerBlock
    torch.manual_seed(seed)
    blk = ConformerBlock(d, heads, ff, kernel, dropout).double()
    with torch.no_grad():
        for name, p in blk.named_parameters():                                # torch's defaults leave biases zero and gains one
            if name.endswith('bias'):
                p.normal_(0, 0.3)
            elif p.dim() == 1:
                p.uniform_(0.5, 1.5)
    return blk


# ---- the references against torch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scale,with_branch,with_mask', [(1.0, True, False), (0.5, True, True), (1.0, False, False)])
def test_res_layernorm_reference_agrees_with_torch(scale, with_branch, with_mask):
    r = np.random.default_rng(1)
    M, Cn = 7, 24
    x, br, dy, dz = (r.standard_normal((M, Cn)) for _ in range(4))
    gm, bt = 1 + 0.3 * r.standard_normal(Cn), r.standard_normal(Cn)
    mask = cr.drop_mask((M, Cn), 0.3, 77) if with_mask else None
    tx, tb = torch.tensor(x, requires_grad=True), torch.tensor(br, requires_grad=True)
    ln = nn.LayerNorm(Cn).double()
    with torch.no_grad():
        ln.weight.copy_(torch.tensor(gm)), ln.bias.copy_(torch.tensor(bt))
    dropped = tb if mask is None else tb * torch.tensor(mask[0] * float(mask[1]))
    tz = tx + scale * dropped if with_branch else tx + 0
    ty = ln(tz)
    (ty * torch.tensor(dy)).sum().add((tz * torch.tensor(dz)).sum()).backward()
    z, y, mean, rstd = cr.res_layernorm_fwd(x, br if with_branch else None, scale, mask, gm, bt, ln.eps)
    _close(z, tz.detach().numpy()), _close(y, ty.detach().numpy())
    _close(mean, tz.detach().numpy().mean(-1)), _close(rstd, 1 / np.sqrt(tz.detach().numpy().var(-1) + ln.eps))
    dx, dbr, dg, db = cr.res_layernorm_bwd(dy, dz, x, br if with_branch else None, scale, mask, gm, mean, rstd)
    _close(dx, tx.grad.numpy()), _close(dg, ln.weight.grad.numpy()), _close(db, ln.bias.grad.numpy())
    if with_branch:
        _close(dbr, tb.grad.numpy())
        if mask is not None:
            assert (dbr[~mask[0]] == 0).all() and (z[~mask[0]] == x[~mask[0]]).all()
    else:
        assert dbr is None
    only_dz = cr.res_layernorm_bwd(None, dz, x, br if with_branch else None, scale, mask, gm, mean, rstd)
    assert only_dz[2] is None and only_dz[3] is None and np.array_equal(only_dz[0], dz)


def test_bias_swish_dropout_reference_agrees_with_torch():
    r = np.random.default_rng(2)
    a, dh, b = r.standard_normal((5, 12)) * 3, r.standard_normal((5, 12)), r.standard_normal(12)
    mask = cr.drop_mask((5, 12), 0.4, 5)
    ta, tb = torch.tensor(a, requires_grad=True), torch.tensor(b, requires_grad=True)
    th = F.silu(ta + tb) * torch.tensor(mask[0] * float(mask[1]))
    (th * torch.tensor(dh)).sum().backward()
    _close(cr.bias_swish_dropout_fwd(a, b, mask), th.detach().numpy())
    da, db = cr.bias_swish_dropout_bwd(dh, a, b, mask)
    _close(da, ta.grad.numpy()), _close(db, tb.grad.numpy())
    _close(cr.bias_swish_dropout_fwd(a, b, None), F.silu(ta + tb).detach().numpy())


@pytest.mark.parametrize('B,T,d,K', [(2, 9, 8, 3), (1, 4, 12, 7), (3, 1, 8, 5), (2, 40, 16, 31)])
def test_conv_module_reference_agrees_with_torch(B, T, d, K):
    """F.glu, nn.Conv1d (depthwise, zero padding), nn.LayerNorm and F.silu composed, forward and every gradient; both tap orders"""
    torch.manual_seed(K)
    dw, ln = nn.Conv1d(d, d, K, padding=K // 2, groups=d).double(), nn.LayerNorm(d).double()
    with torch.no_grad():
        ln.weight.uniform_(0.5, 1.5), ln.bias.normal_(0, 0.3)
    a = torch.randn(B, T, 2 * d, dtype=torch.float64, requires_grad=True)
    u = F.silu(ln(dw(F.glu(a, dim=-1).transpose(1, 2)).transpose(1, 2)))
    du = torch.randn_like(u)
    u.backward(du)
    args = (a.detach().numpy(), dw.weight.detach().numpy().reshape(d, K), dw.bias.detach().numpy(), ln.weight.detach().numpy(),
            ln.bias.detach().numpy(), ln.eps)
    for reverse in (False, True):
        _close(cr.conv_module_fwd(*args, reverse=reverse), u.detach().numpy())
        got = cr.conv_module_bwd(du.numpy(), *args, reverse=reverse)
        for g, w, name in zip(got, (a.grad, dw.weight.grad.reshape(d, K), dw.bias.grad, ln.weight.grad, ln.bias.grad),
                              ('da', 'dw', 'dwb', 'dgamma', 'dbeta')):
            _close(g, w.numpy(), name)


@pytest.mark.parametrize('B,T,d,heads,ff,K', [(2, 9, 16, 2, 24, 5), (1, 33, 32, 4, 40, 7), (3, 2, 24, 3, 16, 3)])
def test_block_reference_agrees_with_the_torch_block(B, T, d, heads, ff, K):
    blk = _block(d, heads, ff, K, seed=T).eval()
    x = torch.randn(B, T, d, dtype=torch.float64, requires_grad=True)
    y = blk(x)
    gy = torch.randn_like(y)
    y.backward(gy)
    P = {k: v.detach().numpy() for k, v in blk.state_dict().items()}
    assert set(P) == set(SUFFIXES)
    yr, dx, G = cr.block(x.detach().numpy(), P, heads, dy=gy.numpy())
    _close(yr, y.detach().numpy(), 'y'), _close(dx, x.grad.numpy(), 'dx')
    assert set(G) == set(P)
    for k, p in blk.named_parameters():
        _close(G[k], p.grad.numpy(), k)
    _close(cr.block(x.detach().numpy(), P, heads), yr)


def test_block_reference_gradients_against_finite_differences():
    """one tiny case, dropout masks present: every gradient of the reference against a central difference along a random direction"""
    d, heads, B, T = 8, 2, 2, 5
    blk = _block(d, heads, 12, 3, seed=9)
    r = np.random.default_rng(4)
    P = {k: v.detach().numpy() for k, v in blk.state_dict().items()}
    x, gy = r.standard_normal((B, T, d)), r.standard_normal((B, T, d))
    masks = {s: cr.drop_mask((B, T, 12 if s.endswith('_in') else d), 0.25, 100 + i) for i, s in enumerate(cr.SITES)}
    assert all(0 < m[0].mean() < 1 for m in masks.values())
    _, dx, G = cr.block(x, P, heads, masks=masks, dy=gy)

    def loss(xv, Pv):
        return float((cr.block(xv, Pv, heads, masks=masks) * gy).sum())

    h = 1e-6
    for name, grad in [('x', dx)] + sorted(G.items()):
        v = r.standard_normal(grad.shape)
        if name == 'x':
            num = (loss(x + h * v, P) - loss(x - h * v, P)) / (2 * h)
        else:
            num = (loss(x, dict(P, **{name: P[name] + h * v})) - loss(x, dict(P, **{name: P[name] - h * v}))) / (2 * h)
        ana = float((grad * v).sum())
        assert abs(num - ana) <= 1e-6 * max(1.0, abs(ana)), (name, num, ana)


def test_float32_evaluation_lands_near_and_not_on_the_float64_one():
    r = np.random.default_rng(3)
    a, du = r.standard_normal((2, 20, 64)).astype(np.float32), r.standard_normal((2, 20, 32)).astype(np.float32)
    w, wb, gm, bt = (r.standard_normal(s).astype(np.float32) for s in ((32, 7), (32,), (32,), (32,)))
    f64, f32 = cr.conv_module_bwd(du, a, w, wb, gm, bt), cr.conv_module_bwd(du, a, w, wb, gm, bt, dtype=np.float32)
    for p, q in zip(f32, f64):
        assert p.dtype == np.float32
        err = np.abs(p.astype(np.float64) - q).max()
        assert 0 < err < 1e-3 * max(1.0, np.abs(q).max())


def test_left_to_right_sums_are_the_same_formulas_in_another_order():
    r = np.random.default_rng(8)
    x, dy = r.standard_normal((6, 512)).astype(np.float32), r.standard_normal((6, 512)).astype(np.float32)
    gm, bt = np.ones(512, np.float32), np.zeros(512, np.float32)

    def both(dtype):
        y, mean, rstd = cr.layernorm_fwd(x, gm, bt, 1e-5, dtype)
        return (y, mean, rstd) + cr.layernorm_bwd(dy, x, gm, mean, rstd, dtype)
    with cr.sequential_sums():
        seq64, seq32 = both(np.float64), both(np.float32)
    for a, b, c, d in zip(both(np.float64), seq64, both(np.float32), seq32):
        assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(a).max())
        assert c.dtype == d.dtype == np.float32 and np.abs(c - d).max() <= 1e-4 * max(1.0, np.abs(a).max())
    assert not np.array_equal(both(np.float32)[1], seq32[1])                   # the order matters in float32
    assert not cr._SEQUENTIAL[0]


# ---- the restated mask --------------------------------------------------------------------------------------------------------------
def _block_seeds(manual_seed, p):
    from salsa_amd.crnn.conformer import draw_seed
    torch.manual_seed(manual_seed)
    return [draw_seed(p) for _ in cr.SITES]


def test_restated_mask_is_seeded_and_drops_the_quantised_share():
    n = 1 << 16
    assert cr.drop_threshold(0.0) == 0 and cr.drop_threshold(0.5) == 32768 and cr.drop_threshold(0.2) == 13107
    assert cr.drop_threshold(0.99999) == 65535 and float(cr.drop_scale(0.5)) == 2.0 and float(cr.drop_scale(0.0)) == 1.0
    assert cr.drop_mask((n,), 0.0, 5)[0].all()
    a, b = cr.drop_mask((n,), 0.2, cr.GPU_TEST_SEEDS[0])[0], cr.drop_mask((n,), 0.2, cr.GPU_TEST_SEEDS[0])[0]
    assert np.array_equal(a, b)
    assert not np.array_equal(a, cr.drop_mask((n,), 0.2, cr.GPU_TEST_SEEDS[1])[0])
    # the two elements of a pair take different halves of one hash
    h = cr.drop_hash(np.arange(4, dtype=np.uint64), 9)
    keep = cr.drop_mask((8,), 0.5, 9)[0]
    assert np.array_equal(keep[0::2], (h & np.uint64(0xFFFF)) >= 32768) and np.array_equal(keep[1::2], (h >> np.uint64(16)) >= 32768)
    seeds = list(cr.GPU_TEST_SEEDS) + _block_seeds(cr.GPU_BLOCK_MANUAL_SEED, 0.2)
    assert _block_seeds(cr.GPU_BLOCK_MANUAL_SEED, 0.2) == _block_seeds(cr.GPU_BLOCK_MANUAL_SEED, 0.2) and len(set(seeds)) == len(seeds)
    for p in (0.2, 0.5):
        q = cr.drop_threshold(p) / 65536.0
        for seed in seeds:
            dropped = n - int(cr.drop_mask((n,), p, seed)[0].sum())
            assert abs(dropped - n * q) <= 5 * np.sqrt(n * q * (1 - q)), (p, seed, dropped)


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def test_zero_layers_is_the_parent_model_bit_for_bit():
    torch.manual_seed(3)
    plain = SeldCRNN().eval()
    torch.manual_seed(3)
    zero = SeldCRNN(n_conformer_layers=0).eval()
    assert list(plain.state_dict()) == list(zero.state_dict()) and not any('conformer' in k for k in zero.state_dict())
    assert len(zero.decoder.conformer) == 0
    x = torch.randn(1, 7, 32, 200, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        a, b = plain(x), zero(x)
    assert all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize('decoder_type,d', [('bigru', 512), ('gru', 256)])
def test_two_layers_keys_shapes_and_checkpoint_round_trip(decoder_type, d):
    from salsa_amd.crnn.checkpoint import to_reference_key
    model = SeldCRNN(decoder_type=decoder_type, n_conformer_layers=2)
    sd = model.state_dict()
    want = {'decoder.conformer.%d.%s' % (i, s) for i in range(2) for s in SUFFIXES}
    assert {k for k in sd if 'conformer' in k} == want and len(want) == 60
    assert set(sd) - want == set(SeldCRNN(decoder_type=decoder_type).state_dict())
    shapes = {'norm_ff1.weight': (d,), 'ff1_w1.weight': (1024, d), 'ff1_w1.bias': (1024,), 'ff1_w2.weight': (d, 1024), 'ff1_w2.bias': (d,),
              'mha.in_proj_weight': (3 * d, d), 'mha.in_proj_bias': (3 * d,), 'mha.out_proj.weight': (d, d), 'conv_p1.weight': (2 * d, d),
              'conv_p1.bias': (2 * d,), 'conv_dw.weight': (d, 1, 7), 'conv_dw.bias': (d,), 'conv_norm.weight': (d,),
              'conv_p2.weight': (d, d), 'ff2_w1.weight': (1024, d), 'ff2_w2.weight': (d, 1024), 'norm_out.bias': (d,)}
    for i in range(2):
        for s, shape in shapes.items():
            assert tuple(sd['decoder.conformer.%d.%s' % (i, s)].shape) == shape, s
        blk = model.decoder.conformer[i]
        assert blk.mha.head_dim == d // 8 and blk.drop.p == 0.1 and blk.mha.dropout == 0.0 and blk.conv_dw.padding == (3,)
        assert all(m.eps == 1e-5 for m in blk.modules() if isinstance(m, nn.LayerNorm))
    assert all(to_reference_key(k) == k for k in want)
    other = SeldCRNN(decoder_type=decoder_type, n_conformer_layers=2)
    assert other.load_reference_state_dict(model.reference_state_dict()) == ([], [])
    plain = {k: v for k, v in model.reference_state_dict().items() if 'conformer' not in k}    # what a reference checkpoint holds
    missing, unexpected = other.load_reference_state_dict(plain, strict=False)
    assert set(missing) == want and unexpected == []


@pytest.mark.parametrize('decoder_type', ['bigru', 'gru', 'lstm', 'bilstm'])
def test_cpu_decoder_equals_the_reference_composition(decoder_type):
    torch.manual_seed(11)
    dec = Decoder(64, 3, 32, decoder_type, 'avg', n_conformer_layers=2, conformer_heads=4, conformer_ff=48, conformer_kernel=5).eval()
    d = 64 if decoder_type.startswith('bi') else 32
    assert all(b.mha.embed_dim == d and b.ff1_w1.out_features == 48 and b.conv_dw.kernel_size == (5,) for b in dec.conformer)
    feat = torch.randn(2, 64, 9, 5)
    out = dec(feat)
    seq, _ = dec.rnn(feat.mean(dim=3).transpose(1, 2))
    seq = seq.detach().numpy()
    for b in dec.conformer:
        seq = cr.block(seq, {k: v.numpy() for k, v in b.state_dict().items()}, 4)
    want = dec.event(torch.tensor(seq, dtype=torch.float32))
    torch.testing.assert_close(out['event_frame_logit'], want, rtol=1e-4, atol=1e-5)


def test_bad_keywords_are_refused():
    with pytest.raises(ValueError, match='conformer_heads'):
        SeldCRNN(n_conformer_layers=1, conformer_heads=7)                     # 512 % 7
    with pytest.raises(ValueError, match='conformer_heads'):
        Decoder(512, 12, 256, 'gru', 'avg', n_conformer_layers=2, conformer_heads=6)
    with pytest.raises(ValueError, match='n_conformer_layers'):
        SeldCRNN(n_conformer_layers=-1)
    for kernel in (4, 1, 33, 0):
        with pytest.raises(ValueError, match='conformer_kernel'):
            Decoder(512, 12, 256, 'bigru', 'avg', n_conformer_layers=1, conformer_kernel=kernel)
    with pytest.raises(ValueError, match='n_attn_layers and n_conformer_layers'):
        SeldCRNN(n_attn_layers=1, n_conformer_layers=1)
    with pytest.raises(NotImplementedError):                                   # the refusal this stage does not lift
        SeldCRNN(decoder_type='transformer', n_conformer_layers=2)
    for decoder_type in ('gru', 'lstm', 'bilstm'):
        assert len(Decoder(64, 3, 32, decoder_type, 'max', n_conformer_layers=1, conformer_heads=4, conformer_ff=8).conformer) == 1


def test_trainer_step_moves_every_conformer_parameter():
    from salsa_amd.crnn.train import Trainer, synthetic_batch
    tr = Trainer('cpu', amp_dtype=None, n_conformer_layers=2, decoder_size=32, conformer_heads=4, conformer_ff=64)
    assert tr.conformer == dict(n_conformer_layers=2, conformer_heads=4, conformer_ff=64, conformer_kernel=7, conformer_dropout=0.1)
    named = {k: p for k, p in tr.raw_model.named_parameters() if '.conformer.' in k}
    assert len(named) == 60
    before = {k: p.detach().clone() for k, p in named.items()}
    x, sed, doa = synthetic_batch(2, 'cpu', n_frames=64)
    loss = tr.train_step(x, sed, doa)[0]
    assert torch.isfinite(loss)
    for k, p in named.items():
        assert p.grad is not None and float(p.grad.abs().max()) > 0, k
        assert not torch.equal(p.detach(), before[k]), k
    p, dd = tr.infer(x)
    assert p.shape == (2, 8, 12) and dd.shape == (2, 8, 36) and bool(torch.isfinite(dd).all())


def test_dropout_off_covers_the_blocks():
    from salsa_amd.crnn.testing import dropout_off
    dec = Decoder(64, 3, 32, 'bigru', 'avg', n_conformer_layers=2, conformer_heads=4, conformer_ff=48, conformer_dropout=0.5).train()
    assert all(isinstance(b.drop, nn.Dropout) and b.drop.p == 0.5 and b.mha.dropout == 0.0 for b in dec.conformer)
    assert sum(isinstance(m, nn.Dropout) for b in dec.conformer for m in b.modules()) == 2     # every site of a block reads block.drop
    feat = torch.randn(2, 64, 9, 5)
    with dropout_off(dec):
        assert all(b.drop.p == 0.0 for b in dec.conformer)
        a, b = dec(feat)['event_frame_logit'], dec(feat)['event_frame_logit']
    assert torch.equal(a, b)
    assert all(b.drop.p == 0.5 for b in dec.conformer)
    assert not torch.equal(dec(feat)['event_frame_logit'], dec(feat)['event_frame_logit'])


def test_checkpoints_store_the_stage_and_resume_checks_it(tmp_path):
    from salsa_amd.crnn import fit
    from salsa_amd.crnn.train import Trainer
    kw = dict(amp_dtype=None, decoder_size=32, n_conformer_layers=2, conformer_heads=4, conformer_ff=64)
    tr = Trainer('cpu', **kw)
    loader = types.SimpleNamespace(seed=5)
    path = str(tmp_path / 'epoch=000.ckpt')
    fit._save(path, tr, loader, 0, 1, dict(steps=[]), None)
    ckpt = torch.load(path, map_location='cpu', weights_only=False)
    assert [ckpt[k] for k in ('n_conformer_layers', 'conformer_heads', 'conformer_ff', 'conformer_kernel', 'conformer_dropout')] == [2, 4, 64, 7, 0.1]
    assert ckpt['n_attn_layers'] == 0 and 'decoder.conformer.1.norm_out.bias' in ckpt['state_dict']
    assert fit._load(path, tr, loader)['epoch'] == 0
    with pytest.raises(ValueError, match='n_conformer_layers'):
        fit._load(path, Trainer('cpu', amp_dtype=None, decoder_size=32), loader)
    for key, value in (('conformer_heads', 8), ('conformer_ff', 32), ('conformer_kernel', 5), ('conformer_dropout', 0.2)):
        with pytest.raises(ValueError, match=key):
            fit._load(path, Trainer('cpu', **dict(kw, **{key: value})), loader)
    plain = Trainer('cpu', amp_dtype=None, decoder_size=32)
    fit._save(path, plain, loader, 0, 1, dict(steps=[]), None)
    assert torch.load(path, map_location='cpu', weights_only=False)['n_conformer_layers'] == 0
    assert fit._load(path, plain, loader)['epoch'] == 0
    with pytest.raises(ValueError, match='n_conformer_layers'):
        fit._load(path, tr, loader)


def test_packed_parameters_leave_the_blocks_alone():
    torch.manual_seed(3)
    m = SeldCRNN(n_conformer_layers=1)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    params = dict(m.named_parameters())
    assert m.pack_parameters() is m
    after = m.state_dict()
    assert list(before) == list(after) and all(torch.equal(before[k], after[k]) for k in before)
    assert all(p is dict(m.named_parameters())[k] for k, p in params.items())
    assert all(p.is_contiguous() for k, p in params.items() if '.conformer.' in k)


def _grad_sync_worker(rank, world, port):
    import torch.distributed as dist
    from salsa_amd.crnn.grad_sync import BucketedGradSync
    os.environ['MASTER_ADDR'], os.environ['MASTER_PORT'] = '127.0.0.1', str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from salsa_amd.crnn.model import ConformerBlock
    torch.manual_seed(rank)                                                    # replicas that do NOT start identical
    blk = ConformerBlock(16, 2, 24, 5, dropout=0.0)
    sync = BucketedGradSync(list(blk.parameters()), bucket_mb=1e-3, module=blk)
    assert len(sync.buckets) >= 3
    sync.broadcast_parameters(0)
    flat = torch.cat([p.detach().flatten() for p in blk.parameters()])
    both = [torch.empty_like(flat) for _ in range(world)]
    dist.all_gather(both, flat)
    assert torch.equal(both[0], both[1])
    x = torch.randn(2, 7, 16, generator=torch.Generator().manual_seed(10 + rank))
    sync.begin()
    blk(x).square().mean().backward()
    sync.finish()
    got = torch.cat([p.grad.flatten() for p in blk.parameters()])
    blk.zero_grad(set_to_none=True)
    with sync.no_sync():
        blk(x).square().mean().backward()
    local = torch.cat([p.grad.flatten() for p in blk.parameters()])
    dist.all_reduce(local)
    assert torch.allclose(got, local / world, rtol=1e-5, atol=1e-7) and float(got.abs().max()) > 0
    sync.remove()
    dist.barrier()
    dist.destroy_process_group()


def test_bucketed_grad_sync_averages_the_blocks_gradients():
    """grad_sync.BucketedGradSync over a ConformerBlock's 30 parameters on a two-rank gloo job: the parameters follow rank 0 and every
    gradient is the average over the ranks"""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_grad_sync_worker, args=(2, port), nprocs=2, join=True)


# ---- the plumbing -------------------------------------------------------------------------------------------------------------------
NEW_EXPORTS = tuple('salsa_nn_%s_%s' % (f, s) for f in ('res_layernorm', 'bias_swish_dropout', 'conv_module')
                    for s in ('supported', 'ws_bytes', 'fwd', 'bwd'))


def test_exports_build_list_and_switch():
    text = open(os.path.join(_lib.INCLUDE_DIR, 'salsa_nn.h')).read()
    for name in NEW_EXPORTS:
        assert name + '(' in text and name in _lib.NN_EXPORTS
    protos = _lib.PROTOTYPES['salsa_nn.h']
    assert protos['salsa_nn_conv_module_ws_bytes'] == (C.c_size_t, [C.c_int] * 4)
    assert protos['salsa_nn_res_layernorm_fwd'][1][:5] == [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_uint32]
    assert os.path.join(_lib.CSRC_DIR, 'conformer.hip') in _lib.build_command()
    assert open(os.path.join(_lib.CSRC_DIR, 'conformer.hip')).read().split('\n#include')[1].strip() == '"build_guard.h"'
    assert 'SALSA_NN_CONV_MODULE_TILE 16' in text
    from salsa_amd.crnn import conformer
    assert conformer.HIP_CONFORMER is True or os.environ.get('SALSA_HIP_CONFORMER') == '0'
    assert 'SALSA_HIP_CONFORMER' in open(os.path.join(os.path.dirname(_lib.INCLUDE_DIR), 'README.md')).read()


def test_launchers_refuse_before_any_device_call():
    L = _lib.load()
    buf = np.zeros(64, np.float32)
    p = C.c_void_p(buf.ctypes.data)                                            # a HOST pointer: a launch with it would be an error
    # res_layernorm
    assert [L.salsa_nn_res_layernorm_supported(M, Cn) for M, Cn in ((1, 256), (9600, 512), (0, 256), (4, 128), (4, 384), (1 << 23, 512))] == [1, 1, 0, 0, 0, 0]
    assert L.salsa_nn_res_layernorm_supported((1 << 23) - 1, 512) == 1          # 2^32 elements are refused, one row fewer is taken
    assert L.salsa_nn_res_layernorm_ws_bytes(7, 256) == 2 * 2 * 256 * 4 and L.salsa_nn_res_layernorm_ws_bytes(5, 300) == 0
    fwd = lambda a, M=4, Cn=256, pd=0.0, eps=1e-5: L.salsa_nn_res_layernorm_fwd(a[0], a[1], 1.0, pd, 3, *a[2:], M, Cn, eps, None)   # noqa: E731
    assert fwd([None] + [p] * 7) == -1 and fwd([p] * 4 + [None, None, p, p]) == -1          # no x; neither output
    for hole in (2, 3, 6, 7):                                                  # with y_out: gamma, beta, mean, rstd
        args = [p] * 8
        args[hole] = None
        assert fwd(args) == -1
    for M, Cn in ((0, 256), (4, 128), (-3, 512), (1 << 23, 512)):
        assert fwd([p] * 8, M, Cn) == -1
    assert fwd([p] * 8, pd=1.0) == -1 and fwd([p] * 8, pd=-0.1) == -1 and fwd([p] * 8, eps=-1.0) == -1
    bwd = lambda a, M=4, Cn=256, wsb=1 << 20: L.salsa_nn_res_layernorm_bwd(*a[:4], 0.5, 0.2, 3, *a[4:], wsb, M, Cn, None)   # noqa: E731
    # (dy, dz_in, x, branch | gamma, mean, rstd, dx, dbranch, dgamma, dbeta, ws)
    for holes in ((2,), (7,), (0, 1), (3,), (4,), (5,), (6,), (9,), (10,), (11,)):   # (3: dbranch without a branch)
        args = [p] * 12
        for hole in holes:
            args[hole] = None
        assert bwd(args) == -1, holes
    assert bwd([p] * 12, 4, 128) == -1 and bwd([p] * 12, 0, 256) == -1
    assert bwd([p] * 12, wsb=16) == -5
    # bias_swish_dropout
    assert [L.salsa_nn_bias_swish_dropout_supported(M, Cn) for M, Cn in ((1, 4), (130, 4096), (3, 6), (3, 4100), (0, 8), (1 << 20, 4096))] == [1, 1, 0, 0, 0, 0]
    assert L.salsa_nn_bias_swish_dropout_ws_bytes(7, 1024) == 2 * 1024 * 4 and L.salsa_nn_bias_swish_dropout_ws_bytes(1 << 16, 8) == 64 * 8 * 4
    assert L.salsa_nn_bias_swish_dropout_fwd(None, p, p, 2, 8, 0.1, 1, None) == -1 and L.salsa_nn_bias_swish_dropout_fwd(p, p, None, 2, 8, 0.1, 1, None) == -1
    assert L.salsa_nn_bias_swish_dropout_fwd(p, p, p, 2, 6, 0.1, 1, None) == -1 and L.salsa_nn_bias_swish_dropout_fwd(p, p, p, 2, 8, 1.0, 1, None) == -1
    for hole in (0, 1, 3, 5):                                                  # (dh, a, bias, da, dbias, ws): dbias without ws
        args = [p] * 6
        args[hole] = None
        assert L.salsa_nn_bias_swish_dropout_bwd(*args, 1 << 20, 2, 8, 0.1, 1, None) == -1
    assert L.salsa_nn_bias_swish_dropout_bwd(*([p] * 6), 1 << 20, 2, 10, 0.1, 1, None) == -1
    assert L.salsa_nn_bias_swish_dropout_bwd(*([p] * 6), 8, 2, 8, 0.1, 1, None) == -5
    # conv_module
    assert [L.salsa_nn_conv_module_supported(T, d, K) for T, d, K in ((1, 256, 3), (512, 512, 31), (513, 512, 7), (0, 256, 7), (40, 128, 7),
                                                                       (40, 512, 4), (40, 512, 33), (40, 512, 1))] == [1, 1, 0, 0, 0, 0, 0, 0]
    assert L.salsa_nn_conv_module_ws_bytes(2, 40, 512, 7) == (2 * 40 * 512 + 10 * 10 * 512) * 4 and L.salsa_nn_conv_module_ws_bytes(2, 600, 512, 7) == 0
    assert L.salsa_nn_conv_module_ws_bytes(32, 300, 256, 31) == (32 * 300 * 256 + 128 * 34 * 256) * 4
    for hole in range(6):
        args = [p] * 6
        args[hole] = None
        assert L.salsa_nn_conv_module_fwd(*args, 1, 40, 256, 7, 1e-5, None) == -1
    for B, T, d, K in ((0, 40, 256, 7), (1, 513, 256, 7), (1, 40, 384, 7), (1, 40, 256, 6), (1, 40, 256, 33), (70000, 4, 256, 3)):
        assert L.salsa_nn_conv_module_fwd(*([p] * 6), B, T, d, K, 1e-5, None) == -1
        assert L.salsa_nn_conv_module_bwd(*([p] * 12), 1 << 30, B, T, d, K, 1e-5, None) == -1
    for hole in range(12):
        args = [p] * 12
        args[hole] = None
        assert L.salsa_nn_conv_module_bwd(*args, 1 << 30, 1, 40, 256, 7, 1e-5, None) == -1
    assert L.salsa_nn_conv_module_bwd(*([p] * 12), 64, 1, 40, 256, 7, 1e-5, None) == -5
