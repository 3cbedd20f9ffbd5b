"""CPU tests of the decoder options (decoder_type gru | bigru | lstm | bilstm, freq_pool avg | max | avg_max): state-dict keys and
eval outputs against the reference SeldDecoder (fixture g24, tools/make_golden_decoders.py), whole-model outputs, a training step
against the reference decoder and loss, the reference's initialisation structure, and the float64 references of
tests/rnn_reference.py against torch.nn.LSTM / nn.GRU, its scan-level (C ABI) functions against its layer functions, and its
inter-layer dropout masks against finite differences."""
import math

import numpy as np
import pytest
import torch

import rnn_reference as rr
from conftest import load_golden

COMBOS = [(dt, fp) for dt in ('gru', 'bigru', 'lstm', 'bilstm') for fp in ('avg', 'max', 'avg_max')]


def _decoder(dt, fp, seed):
    from salsa_amd.crnn.model import Decoder
    from salsa_amd.crnn.testing import seeded_fill
    d = Decoder(512, 12, 256, dt, fp)
    seeded_fill(d, seed)
    return d


@pytest.mark.parametrize('dt,fp', COMBOS)
def test_reference_keys_and_strict_round_trip(dt, fp):
    from salsa_amd.crnn import SeldCRNN
    from salsa_amd.crnn.testing import seeded_fill
    meta, _ = load_golden('g24_decoders')
    src = SeldCRNN(decoder_type=dt, freq_pool=fp)
    seeded_fill(src, meta['weight_seed'])
    sd = src.reference_state_dict()
    dec_keys = {k: list(v.shape) for k, v in sd.items() if k.startswith('decoder.')}
    assert dec_keys == meta['ref_keys']['%s/%s' % (dt, fp)]
    dst = SeldCRNN(decoder_type=dt, freq_pool=fp)
    missing, unexpected = dst.load_reference_state_dict({'state_dict': {k: v.clone() for k, v in sd.items()}}, strict=True)
    assert missing == [] and unexpected == []
    for k, v in dst.state_dict().items():
        assert torch.equal(v, src.state_dict()[k]), k


def test_lstm_keys_pass_through_the_key_map():
    from salsa_amd.crnn.checkpoint import to_reference_key
    for k in ('decoder.lstm.weight_ih_l0', 'decoder.lstm.weight_hh_l1_reverse', 'decoder.lstm.bias_ih_l1', 'decoder.gru.bias_hh_l0'):
        assert to_reference_key(k) == k


@pytest.mark.parametrize('dt,fp', COMBOS)
def test_decoder_forward_matches_reference(dt, fp):
    meta, a = load_golden('g24_decoders')
    d = _decoder(dt, fp, meta['weight_seed']).eval()
    x = torch.randn(*meta['decoder_input_shape'], generator=torch.Generator().manual_seed(meta['decoder_input_seed']))
    with torch.no_grad():
        out = d(x)
    for k in ('event_frame_logit', 'doa_frame_output'):
        np.testing.assert_allclose(out[k].numpy(), a['dec:%s/%s:%s' % (dt, fp, k)], rtol=1e-4, atol=1e-5, err_msg=k)


@pytest.mark.parametrize('dt,fp', [('bilstm', 'avg_max'), ('gru', 'max')])
def test_whole_model_forward_matches_reference(dt, fp):
    from salsa_amd.crnn import SeldCRNN
    from salsa_amd.crnn.testing import seeded_fill
    meta, a = load_golden('g24_decoders')
    m = SeldCRNN(decoder_type=dt, freq_pool=fp)
    seeded_fill(m, meta['weight_seed'])
    m.eval()
    x = torch.randn(*meta['model_input_shape'], generator=torch.Generator().manual_seed(meta['model_input_seed']))
    with torch.no_grad():
        out = m(x)
    for k in ('event_frame_logit', 'doa_frame_output'):
        np.testing.assert_allclose(out[k].numpy(), a['model:%s/%s:%s' % (dt, fp, k)], rtol=1e-4, atol=1e-5, err_msg=k)
    assert out['event_frame_logit'].shape == (2, 8, 12)


def train_labels(meta):
    """the seeded labels of g24's training cases (tools/make_golden_decoders.py draws them so)"""
    g = torch.Generator().manual_seed(meta['train_seed'])
    sed = (torch.rand(2, 12, 12, generator=g) < 0.2).float()
    v = torch.randn(2, 12, 3, 12, generator=g)
    v = v / v.norm(dim=2, keepdim=True)
    return sed, (v * sed[:, :, None, :]).reshape(2, 12, 36)


@pytest.mark.parametrize('dt,fp', [('bilstm', 'max'), ('lstm', 'avg_max')])
def test_decoder_training_step_matches_reference(dt, fp):
    from salsa_amd.crnn.checkpoint import to_reference_key
    from salsa_amd.crnn.loss import seld_loss
    from salsa_amd.crnn.testing import dropout_off
    meta, a = load_golden('g24_decoders')
    d = _decoder(dt, fp, meta['weight_seed']).train()
    sed, doa = train_labels(meta)
    x = torch.randn(*meta['decoder_input_shape'], generator=torch.Generator().manual_seed(meta['decoder_input_seed'])).requires_grad_(True)
    with dropout_off(d):
        loss, sed_l, doa_l = seld_loss(d(x), sed, doa)
        loss.backward()
    case = '%s/%s' % (dt, fp)
    np.testing.assert_allclose([loss.item(), sed_l.item(), doa_l.item()], a['train:%s:loss' % case], rtol=2e-5)
    params = {to_reference_key('decoder.' + k): p for k, p in d.named_parameters()}
    grads = {k: params[k].grad for k in params}
    grads['input'] = x.grad
    n = 0
    for key, st in meta['grad_strides'].items():
        c, name = key.split(':', 1)
        if c != case:
            continue
        got = grads[name].reshape(-1)[::st].numpy()
        ref = a['train:%s:grad:%s' % (case, name)]
        assert np.abs(got - ref).max() <= 2e-4 * np.abs(ref).max() + 1e-9, (name, float(np.abs(got - ref).max()), float(np.abs(ref).max()))
        n += 1
    assert n == (5 if dt == 'bilstm' else 4)


@pytest.mark.parametrize('kind,bidirectional', [('lstm', False), ('lstm', True), ('gru', False), ('gru', True)])
def test_float64_rnn_reference_agrees_with_torch(kind, bidirectional):
    torch.manual_seed(3)
    cls = torch.nn.LSTM if kind == 'lstm' else torch.nn.GRU
    rnn = cls(24, 16, num_layers=2, batch_first=True, bidirectional=bidirectional).double()
    x = torch.randn(3, 9, 24, dtype=torch.float64, requires_grad=True)
    y, _ = rnn(x)
    dy = torch.randn_like(y)
    y.backward(dy)
    params = {k: p.detach().numpy() for k, p in rnn.named_parameters()}
    ry, rg = rr.rnn_forward_backward(kind, params, x.detach().numpy(), dy.numpy(), 2, bidirectional)
    np.testing.assert_allclose(ry, y.detach().numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(rg['input'], x.grad.numpy(), rtol=1e-9, atol=1e-12)
    for k, p in rnn.named_parameters():
        np.testing.assert_allclose(rg[k], p.grad.numpy(), rtol=1e-9, atol=1e-12, err_msg=k)


def _scan_case(kind, seed, T=7, B=3, D=2, H=8, n_in=5):
    G = (4 if kind == 'lstm' else 3) * H
    r = np.random.default_rng(seed)
    return dict(x=r.standard_normal((T, B, n_in)), wih=r.standard_normal((D, G, n_in)) * 0.4, whh=r.standard_normal((D, G, H)) * 0.4,
                bih=r.standard_normal((D, G)) * 0.3, bhh=r.standard_normal((D, G)) * 0.3, dhs=r.standard_normal((T, B, D, H)))


@pytest.mark.parametrize('kind', ['lstm', 'gru'])
def test_scan_level_references_agree_with_the_layer_functions(kind):
    """lstm_scan / gru_scan and their backwards (the C ABI's tensors: gi in, saved planes, dg / dgi / dgh out, direction 1 stored
    at index t) against lstm_layer / gru_layer on the same data: states, every saved plane, and the layer's dx, dW_ih, dW_hh and
    bias gradients formed from the scan's gate gradients, to 1e-12."""
    c = _scan_case(kind, 5)
    x, wih, whh, bih, bhh, dhs = (c[k] for k in ('x', 'wih', 'whh', 'bih', 'bhh', 'dhs'))
    T, B, D, H = dhs.shape
    gi = np.einsum('tbi,dgi->tbdg', x, wih) + bih
    close = lambda a, b, what: np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12, err_msg=what)
    if kind == 'lstm':
        hs, saved = rr.lstm_scan(gi, whh, bhh)
        dg = rr.lstm_scan_backward(dhs, whh, saved)
        assert saved.shape == (T, B, D, 5 * H) and dg.shape == (T, B, D, 4 * H)
        dgi = dgh = dg
    else:
        hs, saved = rr.gru_scan(gi, whh, bhh)
        dgi, dgh = rr.gru_scan_backward(dhs, whh, hs, saved)
        assert saved.shape == (T, B, D, 4 * H) and dgi.shape == dgh.shape == (T, B, D, 3 * H)
    dx_all = 0
    for d in range(D):
        layer, back = (rr.lstm_layer, rr.lstm_layer_backward) if kind == 'lstm' else (rr.gru_layer, rr.gru_layer_backward)
        lhs, cache = layer(x, wih[d], whh[d], bih[d], bhh[d], reverse=d == 1)
        close(hs[:, :, d], lhs, 'hs')
        planes = (2, 3, 4, 5, 6) if kind == 'lstm' else (1, 2, 3, 4)            # cache: (h, c, i, f, g, o, c') / (h, r, z, n, hn)
        for k, idx in enumerate(planes):
            close(saved[:, :, d, k * H:(k + 1) * H], np.stack([cache[t][idx] for t in range(T)]), 'saved plane %d' % k)
        dx, dwih, dwhh, dbih, dbhh = back(x, wih[d], whh[d], dhs[:, :, d], cache, reverse=d == 1)
        hprev = np.stack([cache[t][0] for t in range(T)])
        close(dgi[:, :, d] @ wih[d], dx, 'dx')
        close(np.einsum('tbg,tbi->gi', dgi[:, :, d], x), dwih, 'dwih')
        close(np.einsum('tbg,tbk->gk', dgh[:, :, d], hprev), dwhh, 'dwhh')
        close(dgi[:, :, d].sum((0, 1)), dbih, 'dbih')
        close(dgh[:, :, d].sum((0, 1)), dbhh, 'dbhh')
        # direction 1 really is the time-reversed scan: the same layer on the flipped sequence, flipped back
        if d == 1:
            fhs, _ = layer(x[::-1], wih[d], whh[d], bih[d], bhh[d], reverse=False)
            close(hs[:, :, d], fhs[::-1], 'reverse = forward on the flipped sequence')


@pytest.mark.parametrize('kind', ['lstm', 'gru'])
def test_float32_evaluation_of_the_reference_formulas(kind):
    """dtype=np.float32 computes in float32 (the yardstick of the saturated-gate test) and lands near the float64 result"""
    c = _scan_case(kind, 6)
    gi = np.einsum('tbi,dgi->tbdg', c['x'], c['wih']) + c['bih']
    if kind == 'lstm':
        h64, s64 = rr.lstm_scan(gi, c['whh'], c['bhh'])
        h32, s32 = rr.lstm_scan(gi, c['whh'], c['bhh'], dtype=np.float32)
        g64, g32 = rr.lstm_scan_backward(c['dhs'], c['whh'], s64), rr.lstm_scan_backward(c['dhs'], c['whh'], s32, dtype=np.float32)
        l32, _ = rr.lstm_layer(c['x'], c['wih'][0], c['whh'][0], c['bih'][0], c['bhh'][0], dtype=np.float32)
    else:
        h64, s64 = rr.gru_scan(gi, c['whh'], c['bhh'])
        h32, s32 = rr.gru_scan(gi, c['whh'], c['bhh'], dtype=np.float32)
        g64 = rr.gru_scan_backward(c['dhs'], c['whh'], h64, s64)[0]
        g32 = rr.gru_scan_backward(c['dhs'], c['whh'], h32, s32, dtype=np.float32)[0]
        l32, _ = rr.gru_layer(c['x'], c['wih'][0], c['whh'][0], c['bih'][0], c['bhh'][0], dtype=np.float32)
    assert h32.dtype == s32.dtype == g32.dtype == l32.dtype == np.float32 and h64.dtype == g64.dtype == np.float64
    for a, b in ((h32, h64), (s32, s64), (g32, g64), (l32, h64[:, :, 0])):
        err = float(np.abs(a - b).max())
        assert 0 < err <= 2e-5 * max(1.0, float(np.abs(b).max())), err          # float32, not float64 in disguise


def test_reference_sigmoid_saturates_without_overflow_noise():
    for dt in (np.float32, np.float64):
        y = rr._sig(np.array([-1e4, -103.9, -88.8, 0.0, 16.7, 88.8, 1e4], dtype=dt))
        assert y.dtype == dt and y[0] == 0.0 and y[3] == 0.5 and y[-1] == 1.0 and np.all(np.isfinite(y)) and np.all(np.diff(y) >= 0)


def _masked_case(kind, bidirectional, seed, T=5, B=2, H=8, n_in=6, p=0.3):
    torch.manual_seed(seed)
    cls = torch.nn.LSTM if kind == 'lstm' else torch.nn.GRU
    rnn = cls(n_in, H, num_layers=2, batch_first=True, bidirectional=bidirectional).double()
    params = {k: v.detach().numpy().copy() for k, v in rnn.named_parameters()}
    r = np.random.default_rng(seed)
    D = 2 if bidirectional else 1
    x, dy = r.standard_normal((B, T, n_in)), r.standard_normal((B, T, D * H))
    mask = (r.random((T, B, D * H)) >= p) / (1 - p)
    return params, x, dy, mask


@pytest.mark.parametrize('kind,bidirectional', [('lstm', False), ('lstm', True), ('gru', False), ('gru', True)])
def test_all_ones_masks_reproduce_the_unmasked_reference_bit_for_bit(kind, bidirectional):
    params, x, dy, mask = _masked_case(kind, bidirectional, 8)
    y0, g0 = rr.rnn_forward_backward(kind, params, x, dy, 2, bidirectional)
    y1, g1 = rr.rnn_forward_backward(kind, params, x, dy, 2, bidirectional, masks=[None, np.ones_like(mask)])
    assert np.array_equal(y0, y1) and g0.keys() == g1.keys()
    for k in g0:
        assert np.array_equal(g0[k], g1[k]), k
    y2, g2 = rr.rnn_forward_backward(kind, params, x, dy, 2, bidirectional, masks=[None, mask])
    assert not np.array_equal(y0, y2) and not np.array_equal(g0['input'], g2['input'])


@pytest.mark.parametrize('kind,bidirectional', [('lstm', False), ('lstm', True), ('gru', False), ('gru', True)])
def test_masked_reference_gradients_equal_finite_differences(kind, bidirectional):
    """With a random 0 / (1 / (1 - p)) mask on layer 1's input, the masked reference's input gradient and two weight gradients
    (W_hh of layer 0, behind the mask in the backward; W_ih of layer 1's last direction, which reads the masked input) against
    central differences of its own float64 forward, L = sum(y dy): relative 1e-6 of each gradient's largest element."""
    params, x, dy, mask = _masked_case(kind, bidirectional, 9)
    masks = [None, mask]
    _, g = rr.rnn_forward_backward(kind, params, x, dy, 2, bidirectional, masks=masks)
    loss = lambda prm, xx: float((rr.rnn_forward_backward(kind, prm, xx, dy, 2, bidirectional, masks=masks)[0] * dy).sum())
    eps = 1e-5
    rng = np.random.default_rng(10)

    def fd(get, n):
        """central differences at n random elements of the array get(params, x) returns a writable view of"""
        prm, xx = {k: v.copy() for k, v in params.items()}, x.copy()
        a = get(prm, xx)
        idx = rng.choice(a.size, size=min(n, a.size), replace=False)
        out = np.zeros(len(idx))
        for m, i in enumerate(idx):
            v = a.flat[i]
            a.flat[i] = v + eps
            up = loss(prm, xx)
            a.flat[i] = v - eps
            out[m] = (up - loss(prm, xx)) / (2 * eps)
            a.flat[i] = v
        return idx, out
    last = 'weight_ih_l1' + ('_reverse' if bidirectional else '')
    for name, get, n in (('input', lambda prm, xx: xx, x.size), ('weight_hh_l0', lambda prm, xx: prm['weight_hh_l0'], 40),
                         (last, lambda prm, xx: prm[last], 40)):
        idx, num = fd(get, n)
        ana = g[name].reshape(-1)[idx]
        assert np.abs(num - ana).max() <= 1e-6 * np.abs(g[name]).max(), (name, float(np.abs(num - ana).max()), float(np.abs(g[name]).max()))


def test_float64_freq_pool_reference_tie_and_nan_rules():
    x = np.array([[0.0, 2.0, 2.0, 1.0], [0.0, 0.0, 0.0, 0.0], [1.0, np.nan, 3.0, np.nan], [-1.0, -3.0, -1.0, -2.0]])
    y, am = rr.freq_pool(x, 'max')
    assert list(am) == [1, 0, 1, 0] and y[0] == 2.0 and y[1] == 0.0 and np.isnan(y[2]) and y[3] == -1.0
    y2, _ = rr.freq_pool(x, 'avg_max')
    np.testing.assert_allclose(y2[[0, 1, 3]], x[[0, 1, 3]].mean(-1) + y[[0, 1, 3]])
    dx = rr.freq_pool_backward(np.array([1.0, 2.0, 3.0, 4.0]), am, 4, 'avg_max')
    np.testing.assert_allclose(dx[0], [0.25, 1.25, 0.25, 0.25])
    xt = torch.randn(5, 7, 13, dtype=torch.float64, requires_grad=True)                # tie-free: torch's max picks the same index
    yt = torch.max(xt, dim=2)[0] + xt.mean(dim=2)
    g = torch.randn_like(yt)
    yt.backward(g)
    yr, amr = rr.freq_pool(xt.detach().numpy(), 'avg_max')
    np.testing.assert_allclose(yr, yt.detach().numpy(), rtol=1e-12)
    np.testing.assert_allclose(rr.freq_pool_backward(g.numpy(), amr, 13, 'avg_max'), xt.grad.numpy(), rtol=1e-12)


@pytest.mark.parametrize('dt', ['gru', 'lstm', 'bilstm'])
def test_initialisation_restates_the_reference(dt):
    """init_gru as the reference runs it on these decoders: three row blocks of rows // 3 in every _l{i} weight (uniform
    +-sqrt(3/fan_in); the third block of W_hh orthogonal), zero _l{i} biases; the rows beyond 3 (rows // 3) and every _reverse
    parameter keep torch's default U(+-1/sqrt(H)) -- reverse biases included."""
    from salsa_amd.crnn.model import Decoder
    torch.manual_seed(5)
    rnn = Decoder(512, 12, 256, dt, 'avg').rnn
    H = 256
    bound = 1 / math.sqrt(H)
    for name, p in rnn.named_parameters():
        p = p.detach()
        if name.endswith('_reverse'):
            assert float(p.abs().max()) <= bound, name
            if 'bias' in name:
                assert float(p.abs().max()) > 0, name
            continue
        if 'bias' in name:
            assert float(p.abs().max()) == 0.0, name
            continue
        n = p.shape[0] // 3
        for g in range(3):
            blk = p[g * n:(g + 1) * n]
            if 'weight_hh' in name and g == 2:
                q = blk.double()
                assert float((q.t() @ q - torch.eye(q.shape[1], dtype=torch.float64)).abs().max()) < 1e-5, name
            else:
                b = math.sqrt(3.0 / p.shape[1])
                assert float(blk.abs().max()) <= b and float(blk.abs().max()) > 0.9 * b, (name, g)
        if p.shape[0] > 3 * n:
            assert float(p[3 * n:].abs().max()) <= bound, name
    if dt != 'gru':
        assert rnn.weight_hh_l0.shape == (1024, 256) and 3 * (1024 // 3) == 1023


def test_transformer_is_refused_loudly():
    from salsa_amd.crnn import SeldCRNN
    from salsa_amd.crnn.train import Trainer
    with pytest.raises(NotImplementedError, match='transformer'):
        SeldCRNN(decoder_type='transformer')
    with pytest.raises(NotImplementedError, match='transformer'):
        Trainer('cpu', decoder_type='transformer')


def test_head_width_and_trainer_pass_through():
    from salsa_amd.crnn.train import Trainer
    tr = Trainer('cpu', amp_dtype=None, decoder_type='lstm', freq_pool='max', decoder_size=128)
    dec = tr.raw_model.decoder
    assert dec.decoder_type == 'lstm' and dec.freq_pool == 'max' and dec.lstm.hidden_size == 128 and not dec.lstm.bidirectional
    assert dec.event.fc1.in_features == 128 and not hasattr(dec, 'gru')
    assert Trainer('cpu', amp_dtype=None).raw_model.decoder.decoder_type == 'bigru'


def test_dropout_off_covers_the_lstm():
    from salsa_amd.crnn.model import Decoder
    from salsa_amd.crnn.testing import dropout_off
    d = Decoder(512, 12, 256, 'bilstm', 'avg')
    with dropout_off(d):
        assert d.lstm.dropout == 0.0
    assert d.lstm.dropout == 0.3


def test_new_exports_are_listed():
    from salsa_amd import _lib
    from conftest import ROOT
    import os
    import re
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'salsa_gru.h')).read(), flags=re.S)
    assert set(re.findall(r'\b(salsa_lstm_[a-z_]+)\s*\(', hdr)) == set(_lib.LSTM_EXPORTS) == {'salsa_lstm_scan_fwd', 'salsa_lstm_scan_bwd'}
    assert {'salsa_nn_freq_pool_fwd', 'salsa_nn_freq_pool_bwd'} <= set(_lib.NN_EXPORTS)
    assert os.path.join(ROOT, 'salsa_amd', 'csrc', 'lstm_scan.hip') in _lib.build_command()
