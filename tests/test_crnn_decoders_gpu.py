"""GPU tests of the decoder options: the LSTM scan kernels (salsa_amd/csrc/lstm_scan.hip) and the one-direction GRU through
fused_lstm.rnn_forward against torch.nn.LSTM / nn.GRU, the frequency max / avg_max pools (salsa_nn_freq_pool_fwd / _bwd) against
the float64 reference of tests/rnn_reference.py, the whole model against the reference (fixture g24), bf16 training of every
(decoder_type, freq_pool), and a full bilstm / max training step that reaches neither nn.LSTM nor torch.max."""
import ctypes as C

import numpy as np
import pytest
import torch

import rnn_reference as rr
from conftest import load_golden
from nn_reference import _pool_input

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
COMBOS = [(dt, fp) for dt in ('gru', 'bigru', 'lstm', 'bilstm') for fp in ('avg', 'max', 'avg_max')]


@pytest.mark.parametrize('kind', ['lstm', 'gru'])
@pytest.mark.parametrize('bidirectional', [False, True])
@pytest.mark.parametrize('H', [64, 128, 256])
def test_rnn_forward_matches_torch_forward_and_backward(kind, bidirectional, H):
    """rnn_forward (one HIP scan launch per layer) against torch.nn.LSTM / nn.GRU in float32: outputs and every gradient, with the
    bounds of test_crnn_gpu.py's bigru comparison."""
    from salsa_amd.crnn.fused_lstm import rnn_forward
    torch.manual_seed(H + 2 * bidirectional)
    cls = torch.nn.LSTM if kind == 'lstm' else torch.nn.GRU
    n_in = 2 * H
    for T, B in ((40, 5), (7, 2), (300, 3), (1, 2)):
        rnn = cls(n_in, H, num_layers=2, batch_first=True, bidirectional=bidirectional, dropout=0.0).to(DEV)
        x = torch.randn(B, T, n_in, device=DEV, requires_grad=True)
        ref, _ = rnn(x)
        g = torch.randn_like(ref)
        ref.backward(g)
        ref_grads = [x.grad.clone()] + [p.grad.clone() for p in rnn.parameters()]
        x.grad = None
        rnn.zero_grad()
        out = rnn_forward(rnn, x, training=True)
        out.backward(g)
        got_grads = [x.grad.clone()] + [p.grad.clone() for p in rnn.parameters()]
        assert out.shape == ref.shape
        assert torch.allclose(out, ref, rtol=1e-4, atol=1e-5), (T, B, float((out - ref).abs().max()))
        names = ['input'] + [n for n, _ in rnn.named_parameters()]
        for n, a, b in zip(names, got_grads, ref_grads):
            assert torch.allclose(a, b, rtol=2e-3, atol=2e-4), (T, B, n, float((a - b).abs().max()))


def test_lstm_scan_without_saved_gives_the_same_states():
    from salsa_amd import _lib
    L = _lib.load()
    g = torch.Generator(device=DEV).manual_seed(1)
    for D, H in ((1, 64), (2, 256)):
        T, B = 33, 3
        gi = torch.randn((T, B, D, 4 * H), device=DEV, generator=g)
        whh_t = torch.randn((D, H, 4 * H), device=DEV, generator=g) / H ** 0.5
        bhh = torch.randn((D, 4 * H), device=DEV, generator=g) * 0.1
        hs = [torch.full((T, B, D, H), float('nan'), device=DEV) for _ in range(2)]
        saved = torch.empty((T, B, D, 5 * H), device=DEV)
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for h, sv in ((hs[0], C.c_void_p(saved.data_ptr())), (hs[1], None)):
            rc = L.salsa_lstm_scan_fwd(C.c_void_p(gi.data_ptr()), C.c_void_p(whh_t.data_ptr()), C.c_void_p(bhh.data_ptr()),
                                       C.c_void_p(h.data_ptr()), sv, T, B, D, H, s)
            assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(hs[0], hs[1]) and bool(torch.isfinite(hs[0]).all())
    assert L.salsa_lstm_scan_fwd(None, None, None, None, None, 1, 1, 1, 64, None) == -1
    assert L.salsa_lstm_scan_fwd(C.c_void_p(gi.data_ptr()), C.c_void_p(whh_t.data_ptr()), C.c_void_p(bhh.data_ptr()),
                                 C.c_void_p(hs[0].data_ptr()), None, T, B, D, 96, None) == -1          # H not instantiated
    assert L.salsa_lstm_scan_bwd(None, None, None, None, 1, 1, 1, 64, None) == -1


def test_unidirectional_gru_register_resident_scans():
    """decoder_type 'gru' under bf16 autocast: rnn_forward(half_weights=True) runs the register-resident pair with D = 1; bounds of
    test_register_resident_gru_inference_scan and test_register_resident_gru_training_scan_gradients."""
    from salsa_amd.crnn import fused_lstm
    from salsa_amd.crnn.fused_lstm import rnn_forward
    torch.manual_seed(4)
    gru = torch.nn.GRU(512, 256, num_layers=2, batch_first=True, bidirectional=False, dropout=0.3).to(DEV).eval()
    x = torch.randn(5, 300, 512, device=DEV)
    with torch.no_grad():
        ref = gru(x)[0]
        fast = rnn_forward(gru, x, training=False, half_weights=True)
        fused_lstm.REGISTER_WEIGHTS = False
        try:
            slow = rnn_forward(gru, x, training=False, half_weights=True)                # the float32 streaming scan
        finally:
            fused_lstm.REGISTER_WEIGHTS = True
    torch.testing.assert_close(slow, ref, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(fast, ref, rtol=2e-3, atol=2e-3)
    assert not torch.equal(fast, slow)
    torch.manual_seed(7)
    gru = torch.nn.GRU(512, 256, num_layers=2, batch_first=True, bidirectional=False, dropout=0.0).to(DEV).train()
    ref_m = torch.nn.GRU(512, 256, num_layers=2, batch_first=True, bidirectional=False, dropout=0.0).to(DEV).train()
    ref_m.load_state_dict(gru.state_dict())
    x = torch.randn(6, 80, 512, device=DEV)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya = rnn_forward(gru, xa, training=True, half_weights=True)
    yb = ref_m(xb)[0]
    torch.testing.assert_close(ya, yb, rtol=2e-3, atol=2e-3)
    gy = torch.randn_like(yb)
    ya.backward(gy)
    yb.backward(gy)
    torch.testing.assert_close(xa.grad, xb.grad, rtol=1e-2, atol=2e-3)
    for (n, p), (_, q) in zip(gru.named_parameters(), ref_m.named_parameters()):
        torch.testing.assert_close(p.grad, q.grad, rtol=1e-2, atol=1e-2 * float(q.grad.abs().max()), msg=n)


@pytest.mark.parametrize('mode', ['max', 'avg_max'])
def test_freq_pool_kernels_match_the_float64_reference(mode):
    from salsa_amd import _lib
    L = _lib.load()
    m = {'max': 1, 'avg_max': 2}[mode]
    g = torch.Generator(device=DEV).manual_seed(11)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for W in (8, 12, 13):
        for Cn in (64, 512):
            for kind in ('plain', 'ties', 'nan'):
                N, H = 3, 5
                x = _pool_input(N, Cn, H, W, g, kind)
                ref_y, ref_am = rr.freq_pool(x.float().cpu().numpy(), mode)             # (N, C, H)
                for tm in (1, 0):
                    rows = (H, N, Cn) if tm else (N, H, Cn)
                    y = torch.full(rows, 7.0, device=DEV)
                    am = torch.full(rows, 255, dtype=torch.uint8, device=DEV)
                    assert L.salsa_nn_freq_pool_fwd(C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), C.c_void_p(am.data_ptr()),
                                                    N, H, W, Cn, m, tm, s) == 0
                    gy = torch.randn(rows, device=DEV, generator=g)
                    dx = torch.full((N, Cn, H, W), 3.0, dtype=torch.bfloat16, device=DEV).contiguous(memory_format=torch.channels_last)
                    assert L.salsa_nn_freq_pool_bwd(C.c_void_p(gy.data_ptr()), C.c_void_p(am.data_ptr()), C.c_void_p(dx.data_ptr()),
                                                    N, H, W, Cn, m, tm, s) == 0
                    torch.cuda.synchronize()
                    perm = (2, 0, 1) if tm else (0, 2, 1)                                 # (N, C, H) -> the kernel's row order
                    want_y, want_am = np.transpose(ref_y, perm), np.transpose(ref_am, perm)
                    got_y, got_am = y.cpu().numpy(), am.cpu().numpy().astype(np.int64)
                    assert np.array_equal(got_am, want_am), (W, Cn, kind, tm)
                    assert np.array_equal(np.isnan(got_y), np.isnan(want_y))
                    fin = ~np.isnan(want_y)
                    if mode == 'max':
                        assert np.array_equal(got_y[fin], want_y[fin].astype(np.float32)), (W, Cn, kind, tm)   # exact
                    else:
                        np.testing.assert_allclose(got_y[fin], want_y[fin], rtol=1e-6, atol=1e-6)
                    g_nch = np.transpose(gy.cpu().numpy(), (1, 2, 0) if tm else (0, 2, 1))   # back to (N, C, H)
                    want_dx = rr.freq_pool_backward(g_nch.astype(np.float64), ref_am, W, mode)
                    want_dx = torch.from_numpy(want_dx).float().to(torch.bfloat16).float().numpy()
                    got_dx = dx.float().cpu().numpy()
                    if mode == 'max':
                        assert np.array_equal(got_dx, want_dx), (W, Cn, kind, tm)
                    else:
                        np.testing.assert_allclose(got_dx, want_dx, rtol=2 ** -6, atol=1e-30)   # one bf16 rounding either way


@pytest.mark.parametrize('mode', ['max', 'avg_max'])
def test_freq_pool_gradients_equal_torch_autograd_on_tie_free_input(mode):
    from salsa_amd.crnn import nn_ops
    g = torch.Generator(device=DEV).manual_seed(12)
    N, Cn, H, W = 4, 512, 40, 12
    x = torch.rand((N, Cn, H, W), device=DEV, generator=g).argsort(dim=3).float() - 6                # a permutation of -6..5: no ties
    x = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    xa, xb = x.clone().requires_grad_(True), x.float().clone().requires_grad_(True)
    ya = nn_ops.freq_pool_sequence(xa, mode)
    assert type(ya._base.grad_fn).__name__ == '_FreqPoolBackward'                       # the kernel, not the torch fall-back
    yb = torch.max(xb, dim=3)[0]
    if mode == 'avg_max':
        yb = torch.mean(xb, dim=3) + yb
    yb = yb.transpose(1, 2)
    torch.testing.assert_close(ya, yb, rtol=1e-6, atol=1e-6)
    gy = torch.randn(yb.shape, device=DEV, generator=g)
    ya.backward(gy)
    yb.backward(gy)
    if mode == 'max':
        assert torch.equal(xa.grad.float(), xb.grad.to(torch.bfloat16).float())
    else:
        torch.testing.assert_close(xa.grad.float(), xb.grad, rtol=2 ** -6, atol=1e-30)


@pytest.mark.parametrize('dt,fp', [('bilstm', 'avg_max'), ('gru', 'max')])
def test_gpu_whole_model_matches_reference(dt, fp):
    from salsa_amd.crnn import SeldCRNN
    from salsa_amd.crnn.testing import seeded_fill
    meta, a = load_golden('g24_decoders')
    m = SeldCRNN(decoder_type=dt, freq_pool=fp)
    seeded_fill(m, meta['weight_seed'])
    m = m.to(DEV).eval()
    x = torch.randn(*meta['model_input_shape'], generator=torch.Generator().manual_seed(meta['model_input_seed'])).to(DEV)
    with torch.no_grad():
        out = m(x)
    for k in ('event_frame_logit', 'doa_frame_output'):
        np.testing.assert_allclose(out[k].cpu().numpy(), a['model:%s/%s:%s' % (dt, fp, k)], rtol=2e-3, atol=2e-4, err_msg=k)


@pytest.mark.parametrize('dt,fp', COMBOS)
def test_bf16_training_steps_reduce_loss_for_every_decoder(dt, fp):
    from salsa_amd.crnn.train import Trainer, synthetic_batch
    tr = Trainer(DEV, total_steps=100, decoder_type=dt, freq_pool=fp)
    x, sed, doa = synthetic_batch(4, DEV, seed=1)
    losses = [float(tr.train_step(x, sed, doa)[0]) for _ in range(12)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    p, d = tr.infer(x)
    assert p.shape == (4, 80, 12) and d.shape == (4, 80, 36) and float(p.min()) >= 0 and float(p.max()) <= 1


def test_bilstm_max_training_step_calls_neither_nn_lstm_nor_torch_max(monkeypatch):
    """One full bf16 training step of the bilstm / max model on a (32, 7, 640, 200) batch: no nn.LSTM.forward and no torch.max
    reduction (the decoder runs salsa_lstm_scan and salsa_nn_freq_pool); its loss within 1 % of the same step with the LSTM on
    nn.LSTM and the pool on torch (SALSA_FUSED_LSTM=0 SALSA_HIP_FREQ_POOL=0)."""
    from salsa_amd.crnn import fused_lstm, nn_ops
    from salsa_amd.crnn.loss import seld_loss
    from salsa_amd.crnn.testing import dropout_off
    from salsa_amd.crnn.train import Trainer, synthetic_batch
    calls = {'lstm': 0, 'max': 0}
    real_lstm, real_max = torch.nn.LSTM.forward, torch.max

    def lstm_fwd(self, *a, **k):
        calls['lstm'] += 1
        return real_lstm(self, *a, **k)

    def counting_max(*a, **k):
        if len(a) > 1 or 'dim' in k:
            calls['max'] += 1
        return real_max(*a, **k)
    monkeypatch.setattr(torch.nn.LSTM, 'forward', lstm_fwd)
    monkeypatch.setattr(torch, 'max', counting_max)
    x, sed, doa = synthetic_batch(32, DEV, seed=4)

    def step(fused):
        monkeypatch.setattr(fused_lstm, 'FUSED_LSTM', fused)
        monkeypatch.setattr(nn_ops, 'USE_HIP_FREQ_POOL', fused)
        calls['lstm'] = calls['max'] = 0
        tr = Trainer(DEV, total_steps=10, decoder_type='bilstm', freq_pool='max')
        tr.model.train()
        with dropout_off(tr.raw_model):
            with torch.autocast('cuda', dtype=torch.bfloat16):
                pred = tr.model(tr._input_layout(x))
            loss = seld_loss(pred, sed, doa)[0]
            loss.backward()
        torch.cuda.synchronize()
        return loss.item(), dict(calls)

    fused_loss, fused_calls = step(True)
    torch_loss, torch_calls = step(False)
    assert fused_calls == {'lstm': 0, 'max': 0}, fused_calls
    assert torch_calls['lstm'] == 1 and torch_calls['max'] == 1, torch_calls
    assert np.isfinite(fused_loss) and abs(fused_loss - torch_loss) <= 0.01 * abs(torch_loss), (fused_loss, torch_loss)
