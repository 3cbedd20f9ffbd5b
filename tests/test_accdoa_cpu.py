"""CPU tests of the ACCDOA output format (data.output_format 'accdoa'): the torch restatement of the loss, the SED decision and the
DCASE rows against the reference (fixture g25, tools/make_golden_accdoa.py), a decoder training step against the reference's
(event head: exact-zero gradients where the reference has none), the Trainer option and the new exports."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def loss_inputs(shape, seed):
    """g25 (a)'s seeded inputs (tools/make_golden_accdoa.py draws them so)"""
    B, T, nc = shape
    g = torch.Generator().manual_seed(seed)
    pred = torch.tanh(torch.randn(B, T, 3 * nc, generator=g))
    sed = (torch.rand(B, T, nc, generator=g) < 0.3).float()
    v = torch.randn(B, T, 3, nc, generator=g)
    v = v / v.norm(dim=2, keepdim=True)
    return pred, sed, (v * sed[:, :, None, :]).reshape(B, T, 3 * nc)


def accdoa_output(shape, g):
    """g25 (b) / (c)'s seeded xyz outputs"""
    n, T, c3 = shape
    v = torch.randn(n, T, 3, c3 // 3, generator=g)
    v = v / v.norm(dim=2, keepdim=True) * 0.6 * torch.rand(n, T, 1, c3 // 3, generator=g)
    return v.reshape(n, T, c3).numpy().astype(np.float32)


@pytest.mark.parametrize('i', [0, 1])
def test_torch_loss_matches_reference(i):
    from salsa_amd.crnn import accdoa_loss
    meta, a = load_golden('g25_accdoa')
    shape = tuple(meta['loss_shapes'][i])
    pred, sed, doa_gt = loss_inputs(shape, meta['loss_seed'])
    pred.requires_grad_(True)
    logit = torch.randn(shape, requires_grad=True)
    loss, sed_l, doa_l = accdoa_loss({'event_frame_logit': logit, 'doa_frame_output': pred}, sed, doa_gt)
    key = 'loss:%dx%dx%d' % shape
    np.testing.assert_allclose(loss.item(), a[key + ':loss'][0], rtol=2e-6)
    assert doa_l.item() == loss.item() and sed_l.item() == 0.0
    loss.backward()
    ref = a[key + ':grad']
    assert np.abs(pred.grad.numpy() - ref).max() <= 1e-6 * np.abs(ref).max()
    assert logit.grad is not None and torch.count_nonzero(logit.grad) == 0


def test_loss_value_is_independent_of_the_logits():
    """the zero-gradient link to the logits does no arithmetic on them: non-finite logits change nothing"""
    from salsa_amd.crnn import accdoa_loss
    pred, sed, doa_gt = loss_inputs((2, 5, 12), 1)
    logit = torch.full((2, 5, 12), float('nan'), requires_grad=True)
    loss = accdoa_loss({'event_frame_logit': logit, 'doa_frame_output': pred}, sed, doa_gt)[0]
    assert loss.item() == accdoa_loss({'doa_frame_output': pred}, sed, doa_gt)[0].item()
    loss.backward()
    assert torch.count_nonzero(logit.grad) == 0


def test_sed_from_accdoa_is_bit_equal_to_reference():
    from salsa_amd.crnn.nn_ops import accdoa_sed
    from salsa_amd.crnn.postprocess import sed_from_accdoa
    meta, a = load_golden('g25_accdoa')
    y = accdoa_output(tuple(meta['sed_shape']), torch.Generator().manual_seed(meta['sed_seed']))
    got = sed_from_accdoa(y, 12)
    assert got.dtype == np.float32 and np.array_equal(got, a['sed:out'])
    assert np.array_equal(accdoa_sed(torch.from_numpy(y), 12).numpy(), a["sed:out"])       # (CPU tensors: numpy)


def test_dcase_rows_match_reference_whole_file_and_chunks():
    """sed_from_accdoa per chunk, then combine_chunks, then to_dcase_rows: the reference's order (the norm of an average is not
    the average of the norms, so the overlapping chunks pin it)"""
    from salsa_amd.crnn.postprocess import combine_chunks, sed_from_accdoa, to_dcase_rows
    meta, a = load_golden('g25_accdoa')
    g = torch.Generator().manual_seed(meta['rows_seed'])
    doa = accdoa_output((1, 600, 36), g)
    rows = to_dcase_rows(sed_from_accdoa(doa, 12)[0], doa[0], as_array=True)
    assert rows.shape[0] > 1000 and np.array_equal(rows, a['rows:file'].astype(np.int64))
    doa = accdoa_output((meta['n_chunks'], meta['chunk_len'], 36), g)
    cl, ch = meta['chunk_len'], meta['chunk_hop']
    sed = combine_chunks(sed_from_accdoa(doa, 12), cl, ch)
    rows = to_dcase_rows(sed, combine_chunks(doa, cl, ch), as_array=True)
    assert np.array_equal(rows, a['rows:chunks'].astype(np.int64))
    wrong = to_dcase_rows(sed_from_accdoa(combine_chunks(doa, cl, ch), 12), combine_chunks(doa, cl, ch), as_array=True)
    assert not np.array_equal(wrong, rows)                          # (the fixture tells the two orders apart)


@pytest.mark.parametrize('batched', [True, False])
def test_decoder_training_step_matches_reference(batched, monkeypatch):
    from salsa_amd.crnn import accdoa_loss, model
    from salsa_amd.crnn.checkpoint import to_reference_key
    from salsa_amd.crnn.model import Decoder
    from salsa_amd.crnn.testing import dropout_off, seeded_fill
    monkeypatch.setattr(model, 'BATCHED_HEADS', batched)
    meta, a = load_golden('g25_accdoa')
    d = Decoder(512, 12, 256, 'bigru', 'avg')
    seeded_fill(d, meta['weight_seed'])
    d.train()
    g = torch.Generator().manual_seed(meta['train_seed'])
    sed = (torch.rand(2, 12, 12, generator=g) < 0.2).float()
    v = torch.randn(2, 12, 3, 12, generator=g)
    v = v / v.norm(dim=2, keepdim=True)
    doa = (v * sed[:, :, None, :]).reshape(2, 12, 36)
    x = torch.randn(*meta['decoder_input_shape'], generator=torch.Generator().manual_seed(meta['decoder_input_seed'])).requires_grad_(True)
    with dropout_off(d):
        loss, sed_l, doa_l = accdoa_loss(d(x), sed, doa)
        loss.backward()
    np.testing.assert_allclose(loss.item(), a['train:loss'][0], rtol=2e-5)
    params = {to_reference_key('decoder.' + k): p for k, p in d.named_parameters()}
    grads = {k: p.grad for k, p in params.items()}
    grads['input'] = x.grad
    for name, st in meta['grad_strides'].items():
        got = grads[name].reshape(-1)[::st].numpy()
        ref = a['train:grad:%s' % name]
        assert np.abs(got - ref).max() <= 2e-4 * np.abs(ref).max() + 1e-9, (name, float(np.abs(got - ref).max()))
    assert len(meta['grad_none']) == 4
    for name in meta['grad_none']:                                  # None in the reference: exact zeros here
        assert grads[name] is not None and torch.count_nonzero(grads[name]) == 0, name
    for name, gr in grads.items():
        if name not in meta['grad_none']:
            assert gr is not None and torch.count_nonzero(gr) > 0, name


def test_trainer_output_format():
    from salsa_amd.crnn.postprocess import sed_from_accdoa
    from salsa_amd.crnn.train import Trainer, synthetic_batch
    tr = Trainer('cpu', amp_dtype=None, output_format='accdoa')
    ev0 = {k: p.detach().clone() for k, p in tr.raw_model.decoder.event.named_parameters()}
    x, sed, doa = synthetic_batch(2, 'cpu', n_frames=64)
    loss, sed_l, doa_l = tr.train_step(x, sed, doa)
    assert torch.isfinite(loss) and float(sed_l) == 0.0 and float(doa_l) == float(loss)
    for k, p in tr.raw_model.decoder.event.named_parameters():
        assert torch.count_nonzero(p.grad) == 0 and torch.equal(p.detach(), ev0[k]), k
    prob, xyz = tr.infer(x)
    assert prob.shape == (2, 8, 12) and xyz.shape == (2, 8, 36)
    assert np.array_equal(prob.numpy(), sed_from_accdoa(xyz.numpy(), 12))
    assert Trainer('cpu', amp_dtype=None).output_format == 'reg_xyz'
    with pytest.raises(ValueError, match="reg_xyz, accdoa"):
        Trainer('cpu', amp_dtype=None, output_format='reg_polar')


def test_new_exports_are_listed():
    from salsa_amd import _lib
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'salsa_nn.h')).read(), flags=re.S)
    names = set(re.findall(r'\b(salsa_nn_accdoa_[a-z_]+)\s*\(', hdr))
    assert names == {'salsa_nn_accdoa_loss', 'salsa_nn_accdoa_sed'} and names <= set(_lib.NN_EXPORTS)
    import salsa_amd.crnn as crnn
    assert callable(crnn.accdoa_loss) and callable(crnn.seld_loss)
