"""The decoder options' hand-written kernels at the sizes the project runs, held to the standard of
tests/test_nn_kernels_at_scale_gpu.py: the LSTM scans (salsa_lstm_scan_fwd / _bwd), the one-direction GRU scans and the frequency
max / mean + max pools (salsa_nn_freq_pool_fwd / _bwd) against float64 references, and the inter-layer dropout that
fused_gru.bigru_forward and fused_lstm.rnn_forward place themselves.  Run alone:
python -m pytest -m gpu tests/test_rnn_scans_at_scale_gpu.py -q -s   (-s prints each tensor's max error / bound).

  a  LSTM through rnn_forward, H 64 / 128 / 256, one and two directions, (T, B) = (1, 1), (40, 32) training, (300, 32) 60-s
     inference, against nn.LSTM in float64
  b  the one-direction GRU on the same grid, and the register-resident pair with D = 1 at T = 300, B = 32
  c  the LSTM scans at the C ABI with saturated gates (pre-activations up to +-1e4, a forget gate held at 1 for 300 steps): hs,
     each plane of `saved` (i, f, g, o, c) and dg against the scan-level float64 reference of tests/rnn_reference.py
  d  exactness, tolerance zero: batch invariance, direction independence, repeatability, the outputs' footprint, refused shapes
  e  inter-layer dropout of every decoder with a recorded mask, against the masked float64 reference
  f  the max and mean + max pools at the frequency mean's benchmark maps, on plain and tie-laden input

The bound of a, b, c and e is the one of test_gru_scan_forward_and_every_gradient: the kernel's error against float64 may not
exceed 16 times the error of a float32 evaluation on the CPU (nn.LSTM / nn.GRU in float32; in c the same numpy formulas in
float32) plus 2^-20 of the float64 tensor's rms.  It is measured against the reference, never against the kernel.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import nn_reference as nr
import rnn_reference as rr
from nn_reference import _pool_input

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
NAN_BITS = 0x7FC0BEEF            # a quiet NaN with a payload: what guard regions and unwritten outputs hold


def _lib():
    from salsa_amd import _lib
    return _lib.load()


def _report(what, ratio):
    print('%-66s max err / bound %.3g' % (what, ratio))
    return ratio


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _graph_nodes(y):
    """the autograd node type names reachable from y"""
    seen, names, todo = set(), [], [y.grad_fn]
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names.append(type(f).__name__)
        todo += [n for n, _ in f.next_functions]
    return names


def _bounded(tag, names, got, c32, ref):
    """the bound of test_gru_scan_forward_and_every_gradient, tensor by tensor"""
    for name, a, b32, r in zip(names, got, c32, ref):
        a, b32, r = (torch.as_tensor(v).double().cpu() for v in (a, b32, r))
        assert a.shape == r.shape, (tag, name, a.shape, r.shape)
        assert bool(torch.isfinite(a).all()), (tag, name)
        e = float((a - r).abs().max())
        e32 = float((b32 - r).abs().max())
        bound = 16 * e32 + 2.0 ** -20 * float(r.pow(2).mean().sqrt())      # (0 for dW_hh at T = 1: h0 = 0, exactly)
        _report('%s %s' % (tag, name), e / bound if bound > 0 else e)
        assert e <= bound, (tag, name, e, e32)


# ------------------------------------------------------------------------------------- a, b: through rnn_forward at the sizes that run
def _rnn_case(kind, H, T, B, bidirectional, seed, dropout=0.0, layers=2):
    torch.manual_seed(seed)
    cls = torch.nn.LSTM if kind == 'lstm' else torch.nn.GRU
    rnn = cls(512, H, num_layers=layers, batch_first=True, bidirectional=bidirectional, dropout=dropout)
    x = torch.randn(B, T, 512)
    gy = torch.randn(B, T, (2 if bidirectional else 1) * H)
    return rnn, x, gy


def _names(rnn):
    return ['y', 'dx'] + ['d' + n for n, _ in rnn.named_parameters()]


def _f32_cpu(rnn, x, gy):
    """the yardstick: the torch module itself in float32 on the CPU -> [y, dx, every parameter gradient]"""
    m = copy.deepcopy(rnn).cpu().float().train()
    m.dropout = 0.0
    xr = x.clone().requires_grad_(True)
    y = m(xr)[0]
    y.backward(gy)
    return [y.detach(), xr.grad] + [p.grad for p in m.parameters()]


def _run(rnn, x, gy, half_weights=False, forward=None, training=True):
    """-> ([y, dx, every parameter gradient] on the CPU, y's autograd node names)"""
    from salsa_amd.crnn import fused_lstm, nn_ops
    forward = forward or fused_lstm.rnn_forward
    g = copy.deepcopy(rnn).to(DEV).train()
    xa = x.to(DEV).requires_grad_(True)
    nn_ops.new_backward_generation(DEV)                      # as the model does before every differentiable forward
    y = forward(g, xa, training=training, half_weights=half_weights)
    names = _graph_nodes(y)
    y.backward(gy.to(DEV))
    torch.cuda.synchronize()
    return [y.detach().cpu(), xa.grad.cpu()] + [p.grad.cpu() for p in g.parameters()], names


TB = [(1, 1), (40, 32), (300, 32)]


@pytest.mark.parametrize('TB', TB)
@pytest.mark.parametrize('bidirectional', [False, True])
@pytest.mark.parametrize('H', [64, 128, 256])
def test_lstm_scans_through_rnn_forward_against_float64(H, bidirectional, TB):
    """salsa_lstm_scan_fwd / _bwd as rnn_forward launches them (two layers), output, input gradient and every parameter gradient
    against nn.LSTM in float64; yardstick nn.LSTM in float32 on the CPU."""
    T, B = TB
    rnn, x, gy = _rnn_case('lstm', H, T, B, bidirectional, 40 + H + T + bidirectional)
    y64, g64 = nr.rnn_ref(rnn, x, gy)
    got, nodes = _run(rnn, x, gy)
    assert nodes.count('_LstmScanBackward') == 2 and not [n for n in nodes if 'Rnn' in n], nodes     # the kernel, not nn.LSTM
    _bounded('lstm H=%d D=%d T=%d B=%d' % (H, 1 + bidirectional, T, B), _names(rnn), got, _f32_cpu(rnn, x, gy), [y64] + g64)


@pytest.mark.parametrize('TB', TB)
@pytest.mark.parametrize('H', [64, 128, 256])
def test_one_direction_gru_scans_through_rnn_forward_against_float64(H, TB):
    """decoder_type 'gru': salsa_gru_scan_fwd / _bwd with D = 1 through rnn_forward(half_weights=False), same grid and bound"""
    T, B = TB
    rnn, x, gy = _rnn_case('gru', H, T, B, False, 60 + H + T)
    y64, g64 = nr.rnn_ref(rnn, x, gy)
    got, nodes = _run(rnn, x, gy)
    assert nodes.count('_GruScanBackward') == 2 and not [n for n in nodes if 'Rnn' in n], nodes
    _bounded('gru H=%d D=1 T=%d B=%d' % (H, T, B), _names(rnn), got, _f32_cpu(rnn, x, gy), [y64] + g64)


def test_register_resident_gru_pair_with_one_direction_at_bench_size():
    """salsa_gru_scan_fwd_regw / _bwd_regw with D = 1 (rnn_forward(half_weights=True), H = 256), T = 300, B = 32, against nn.GRU in
    float64 with W_hh rounded to float16; the bound of test_register_resident_gru_pair_at_bench_size (2e-3 relative + 2e-3 rms:
    the float16 rounding of h in the recurrent products, 2^-11 relative per step).  And the no-grad inference scan."""
    from salsa_amd.crnn import fused_gru, fused_lstm
    assert fused_gru.REGISTER_WEIGHTS and fused_lstm.REGISTER_WEIGHTS
    rnn, x, gy = _rnn_case('gru', 256, 300, 32, False, 70)
    y64, g64 = nr.rnn_ref(rnn, x, gy, whh_round=lambda p: p.half().double())
    calls = []
    real = _lib().salsa_gru_scan_fwd_regw

    class Spy:                                              # (the library object is shared: count the register-resident launches)
        def __call__(self, *a):
            calls.append(a[7])                              # D
            return real(*a)
    L = _lib()
    L.salsa_gru_scan_fwd_regw = Spy()
    try:
        got, nodes = _run(rnn, x, gy, half_weights=True)
        assert calls == [1, 1] and nodes.count('_GruScanBackward') == 2, (calls, nodes)
        with torch.no_grad():
            yi = fused_lstm.rnn_forward(copy.deepcopy(rnn).to(DEV).eval(), x.to(DEV), training=False, half_weights=True).cpu()
        assert calls == [1, 1, 1, 1]
    finally:
        L.salsa_gru_scan_fwd_regw = real
    for name, a, r in zip(_names(rnn), got + [yi], [y64] + g64 + [y64]):
        rms = float(r.pow(2).mean().sqrt())
        err = (a.double() - r).abs()
        ratio = float((err / (2e-3 * r.abs() + 2e-3 * rms)).max())
        _report('gru regw H=256 D=1 T=300 B=32 %s' % name, ratio)
        assert ratio <= 1, (name, float(err.max()), rms)


# ------------------------------------------------------------------------------------------------- the scans at the C ABI
def _guarded(shape, dtype=torch.float32, pad=None):
    """-> (buffer, view of `shape` inside it): the buffer holds the NaN pattern, `pad` elements lie before and after the view"""
    n = int(np.prod(shape))
    pad = pad or 4096
    buf = torch.full((n + 2 * pad,), NAN_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    return buf, buf[pad:pad + n].view(shape)


def _footprint(buf, view, what):
    """every element of the view was written with a finite value, no element around it was touched"""
    n, pad = view.numel(), (buf.numel() - view.numel()) // 2
    bits = buf.view(torch.int32)
    assert bool((bits[:pad] == NAN_BITS).all()) and bool((bits[pad + n:] == NAN_BITS).all()), what + ': a guard element changed'
    assert bool(torch.isfinite(view).all()), what + ': an element inside was not written (or is not finite)'


def _lstm_launch(gi, whh, bhh, dhs):
    """salsa_lstm_scan_fwd then _bwd on device tensors, outputs inside guarded buffers (guards of 4H floats at least)
    -> hs, saved, dg"""
    T, B, D, H4 = gi.shape
    H = H4 // 4
    L = _lib()
    whh_t = whh.transpose(1, 2).contiguous()
    pad = max(4096, 5 * H)
    (bh, hs), (bs, saved), (bd, dg) = (_guarded((T, B, D, k * H), pad=pad) for k in (1, 5, 4))
    with torch.cuda.device(DEV):
        assert L.salsa_lstm_scan_fwd(_p(gi), _p(whh_t), _p(bhh), _p(hs), _p(saved), T, B, D, H, _stream()) == 0
        assert L.salsa_lstm_scan_bwd(_p(dhs), _p(whh), _p(saved), _p(dg), T, B, D, H, _stream()) == 0
    torch.cuda.synchronize()
    for b, v, what in ((bh, hs, 'hs'), (bs, saved, 'saved'), (bd, dg, 'dg')):
        _footprint(b, v, 'lstm %s T=%d B=%d D=%d H=%d' % (what, T, B, D, H))
    return hs, saved, dg


def _gru_launch(gi, whh, bhh, dhs):
    """salsa_gru_scan_fwd then _bwd (the float32 streaming pair) -> hs, saved, dgi, dgh, guarded as in _lstm_launch"""
    T, B, D, H3 = gi.shape
    H = H3 // 3
    L = _lib()
    whh_t = whh.transpose(1, 2).contiguous()
    pad = max(4096, 4 * H)
    (bh, hs), (bs, saved), (bi, dgi), (bg, dgh) = (_guarded((T, B, D, k * H), pad=pad) for k in (1, 4, 3, 3))
    with torch.cuda.device(DEV):
        assert L.salsa_gru_scan_fwd(_p(gi), _p(whh_t), _p(bhh), _p(hs), _p(saved), T, B, D, H, _stream()) == 0
        assert L.salsa_gru_scan_bwd(_p(dhs), _p(whh), _p(hs), _p(saved), _p(dgi), _p(dgh), T, B, D, H, _stream()) == 0
    torch.cuda.synchronize()
    for b, v, what in ((bh, hs, 'hs'), (bs, saved, 'saved'), (bi, dgi, 'dgi'), (bg, dgh, 'dgh')):
        _footprint(b, v, 'gru %s T=%d B=%d D=%d H=%d' % (what, T, B, D, H))
    return hs, saved, dgi, dgh


def _scan_inputs(kind, T, B, D, H, seed, sigma=1.0):
    """numpy float32 (gi, whh, bhh, dhs): W_hh uniform in +-1 / sqrt(H) (torch's default range), b_hh = 0.1 randn"""
    G = (4 if kind == 'lstm' else 3) * H
    r = np.random.default_rng(seed)
    gi = (sigma * r.standard_normal((T, B, D, G))).astype(np.float32)
    whh = r.uniform(-1, 1, (D, G, H)).astype(np.float32) / np.float32(H ** 0.5)
    bhh = (0.1 * r.standard_normal((D, G))).astype(np.float32)
    dhs = r.standard_normal((T, B, D, H)).astype(np.float32)
    return gi, whh, bhh, dhs


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


PLANTED = [16.7, -16.7, 88.8, -88.8, 100.0, -100.0, -103.9, 1e4, -1e4]


def _plant(gi, H):
    """the values float32 exp cannot take (it overflows above 88.72 and is denormal below -87.3) and the ones around them, each
    in every gate, spread over steps, samples 0..2 and both directions; sample 3's forget gate is held open (+30) in both
    directions for the whole scan, so its cell state integrates over all T steps"""
    T, B, D, _ = gi.shape
    for k, v in enumerate(PLANTED):
        for gate in range(4):
            t, b, d = (5 + 31 * k + 7 * gate) % T, (k + gate) % 3, (k + gate) % D
            gi[t, b, d, gate * H + (3 * k + gate) % 8:(gate + 1) * H:8] = v
    gi[:, 3, :, H:2 * H] = 30.0
    return gi


@pytest.mark.parametrize('sigma', [1, 8, 40])
@pytest.mark.parametrize('H', [64, 256])
def test_lstm_scans_with_saturated_gates_plane_by_plane(H, sigma):
    """salsa_lstm_scan_fwd / _bwd at the C ABI, T = 300, B = 4, D = 2, on inputs that saturate the gates (see _plant): lstm_sigmoid
    where __expf overflows or underflows, 1 - tanh(c)^2 with a cell state integrated over 300 steps.  hs, each of the five planes
    of saved, and dg against rr.lstm_scan / lstm_scan_backward in float64; yardstick the same functions in float32."""
    T, B, D = 300, 4, 2
    gi, whh, bhh, dhs = _scan_inputs('lstm', T, B, D, H, 80 + H + sigma, sigma=sigma)
    gi = _plant(gi, H)
    h64, s64 = rr.lstm_scan(gi, whh, bhh)
    g64 = rr.lstm_scan_backward(dhs, whh, s64)
    h32, s32 = rr.lstm_scan(gi, whh, bhh, dtype=np.float32)
    g32 = rr.lstm_scan_backward(dhs, whh, s32, dtype=np.float32)
    assert all(np.isfinite(a).all() for a in (h64, s64, g64, h32, s32, g32))
    cmax = float(np.abs(s64[..., 4 * H:]).max())
    print('lstm saturated H=%d sigma=%d: max |c| %.1f, float32 yardstick hs %.3g dg %.3g (rms %.3g)'
          % (H, sigma, cmax, np.abs(h32 - h64).max(), np.abs(g32 - g64).max(), np.sqrt((g64 ** 2).mean())))
    assert cmax > 10                                          # the held-open forget gate did integrate
    hs, saved, dg = _lstm_launch(*_dev(gi, whh, bhh, dhs))    # (asserts every output element finite, every guard untouched)
    planes = 'ifgoc'
    names = ['hs'] + ['saved.' + p for p in planes] + ['dg']
    split = lambda s: [s[..., k * H:(k + 1) * H] for k in range(5)]
    _bounded('lstm saturated H=%d sigma=%d' % (H, sigma), names, [hs] + split(saved) + [dg], [h32] + split(s32) + [g32],
             [h64] + split(s64) + [g64])


def _equal(a, b, what):
    assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.contiguous().view(torch.int32)), what      # bit for bit


@pytest.mark.parametrize('H', [256, 64])
@pytest.mark.parametrize('kind', ['lstm', 'gru'])
def test_scans_are_batch_invariant_direction_independent_and_repeatable(kind, H):
    """One workgroup owns one (sample, direction) and nothing is shared between them, so at T = 40, D = 2, forward and backward:
    the B = 32 launch equals B = 1 launches on samples 0, 17 and 31; D = 2 equals two D = 1 launches (direction 1 being the D = 1
    scan of the time-flipped sequence); a second launch repeats the first.  All bit for bit; every launch's outputs lie in
    NaN-filled buffers whose inside must come out finite and whose guards (>= 4H floats either side) untouched."""
    T, B, D = 40, 32, 2
    launch = _lstm_launch if kind == 'lstm' else _gru_launch
    gi, whh, bhh, dhs = _dev(*_scan_inputs(kind, T, B, D, H, 90 + H))
    full = launch(gi, whh, bhh, dhs)
    outs = ('hs', 'saved', 'dg') if kind == 'lstm' else ('hs', 'saved', 'dgi', 'dgh')
    for a, b, n in zip(full, launch(gi, whh, bhh, dhs), outs):
        _equal(a, b, '%s H=%d repeat %s' % (kind, H, n))
    for s in (0, 17, 31):
        one = launch(gi[:, s:s + 1].contiguous(), whh, bhh, dhs[:, s:s + 1].contiguous())
        for a, b, n in zip(one, full, outs):
            _equal(a, b[:, s:s + 1], '%s H=%d sample %d alone %s' % (kind, H, s, n))
    for d in (0, 1):
        flip = (lambda t: t.flip(0)) if d == 1 else (lambda t: t)
        half = launch(flip(gi[:, :, d:d + 1]).contiguous(), whh[d:d + 1].contiguous(), bhh[d:d + 1].contiguous(),
                      flip(dhs[:, :, d:d + 1]).contiguous())
        for a, b, n in zip(half, full, outs):
            _equal(flip(a).contiguous(), b[:, :, d:d + 1], '%s H=%d direction %d alone %s' % (kind, H, d, n))


@pytest.mark.parametrize('kind,bidirectional', [('lstm', False), ('lstm', True), ('gru', False)])
def test_parameter_gradients_of_two_identical_passes_are_bit_equal(kind, bidirectional):
    """through rnn_forward, T = 40, B = 32, H = 256, the library's default mode (deterministic gradient sums, as a fresh process
    has it): output, input gradient and every parameter gradient of two identical forward + backward passes, bit for bit"""
    from salsa_amd.crnn import nn_ops
    rnn, x, gy = _rnn_case(kind, 256, 40, 32, bidirectional, 95)
    prev = nn_ops._DET_USER[0]
    nn_ops._DET_USER[0] = None
    try:
        first, _ = _run(rnn, x, gy)
        second, _ = _run(rnn, x, gy)
    finally:
        if prev is False:
            nn_ops.set_deterministic(False, DEV)
        else:
            nn_ops._DET_USER[0] = prev
    for n, a, b in zip(_names(rnn), first, second):
        assert torch.equal(a, b), (kind, bidirectional, n)


@pytest.mark.parametrize('kind', ['lstm', 'gru'])
def test_scans_refuse_shapes_they_cannot_run_and_accept_the_largest_batch(kind):
    """T = 0, B = 0, B = 65536, D = 3, H = 96 and a NULL among the required pointers return -1 from the host checks, before any
    launch (the buffers passed are nevertheless large enough for every refused shape).  The largest accepted batch, B = 65535 at
    T = 2, H = 64, D = 2, runs and agrees with the float64 reference on samples 0, 32768 and 65534 (bound as in the saturated
    test: 16 x the float32 evaluation of the same formulas + 2^-20 rms)."""
    L = _lib()
    G = 4 if kind == 'lstm' else 3
    T, B, D, H = 2, 65535, 2, 64
    gi_n, whh_n, bhh_n, dhs_n = _scan_inputs(kind, T, B, D, H, 97)
    gi, whh, bhh, dhs = _dev(gi_n, whh_n, bhh_n, dhs_n)
    big = lambda k: torch.zeros((2 * 65536 * 2 * k * 64,), device=DEV)            # [2][65536][2][k 64]: the largest refused shape
    w3 = torch.zeros((3, G * 96, 96), device=DEV)
    b3 = torch.zeros((3, G * 96), device=DEV)
    a_gi, a_hs, a_sv, a_dg, a_dg2 = big(G), big(1), big(5), big(G), big(G)
    if kind == 'lstm':
        fwd = lambda T, B, D, H, p=(a_gi, w3, b3, a_hs, a_sv): L.salsa_lstm_scan_fwd(*[_p(t) if t is not None else None for t in p], T, B, D, H, _stream())
        bwd = lambda T, B, D, H, p=(a_hs, w3, a_sv, a_dg): L.salsa_lstm_scan_bwd(*[_p(t) if t is not None else None for t in p], T, B, D, H, _stream())
        required = ((a_gi, w3, b3, a_hs), (a_hs, w3, a_sv, a_dg))
    else:
        fwd = lambda T, B, D, H, p=(a_gi, w3, b3, a_hs, a_sv): L.salsa_gru_scan_fwd(*[_p(t) if t is not None else None for t in p], T, B, D, H, _stream())
        bwd = lambda T, B, D, H, p=(a_hs, w3, a_hs, a_sv, a_dg, a_dg2): L.salsa_gru_scan_bwd(*[_p(t) if t is not None else None for t in p], T, B, D, H, _stream())
        required = ((a_gi, w3, b3, a_hs), (a_hs, w3, a_hs, a_sv, a_dg, a_dg2))
    with torch.cuda.device(DEV):
        for shape in ((0, 4, 2, 64), (2, 0, 2, 64), (2, 65536, 2, 64), (2, 4, 3, 64), (2, 4, 2, 96), (-1, 4, 2, 64), (2, -4, 2, 64), (2, 4, 0, 64)):
            assert fwd(*shape) == -1, (kind, 'fwd', shape)
            assert bwd(*shape) == -1, (kind, 'bwd', shape)
        for f, req in zip((fwd, bwd), required):
            for i in range(len(req)):
                p = list(req) + ([a_sv] if f is fwd else [])
                p[i] = None
                assert f(2, 4, 2, 64, p=tuple(p)) == -1, (kind, 'NULL argument', i)
    torch.cuda.synchronize()
    for t in (a_hs, a_sv, a_dg, a_dg2):
        assert not bool(t.any()), 'a refused call wrote'
    del a_gi, a_hs, a_sv, a_dg, a_dg2
    out = (_lstm_launch if kind == 'lstm' else _gru_launch)(gi, whh, bhh, dhs)
    pick = [0, 32768, 65534]
    sub = lambda a: a[:, pick]
    if kind == 'lstm':
        r64 = rr.lstm_scan(sub(gi_n), whh_n, bhh_n)
        r64 = r64 + (rr.lstm_scan_backward(sub(dhs_n), whh_n, r64[1]),)
        r32 = rr.lstm_scan(sub(gi_n), whh_n, bhh_n, dtype=np.float32)
        r32 = r32 + (rr.lstm_scan_backward(sub(dhs_n), whh_n, r32[1], dtype=np.float32),)
        names = ('hs', 'saved', 'dg')
    else:
        r64 = rr.gru_scan(sub(gi_n), whh_n, bhh_n)
        r64 = r64 + rr.gru_scan_backward(sub(dhs_n), whh_n, *r64)
        r32 = rr.gru_scan(sub(gi_n), whh_n, bhh_n, dtype=np.float32)
        r32 = r32 + rr.gru_scan_backward(sub(dhs_n), whh_n, *r32, dtype=np.float32)
        names = ('hs', 'saved', 'dgi', 'dgh')
    _bounded('%s B=65535 T=2 H=64 D=2 samples 0, 32768, 65534' % kind, names, [o[:, pick].cpu() for o in out], r32, r64)


@pytest.mark.parametrize('H', [64, 256])
def test_gru_scans_at_the_c_abi_plane_by_plane(H):
    """salsa_gru_scan_fwd / _bwd at the C ABI, T = 40, B = 32, D = 2: hs, each plane of saved (r, z, n, W_hn h + b_hn), dgi and
    dgh against rr.gru_scan / gru_scan_backward in float64 (nobody else reads saved's layout but the backward kernel)"""
    T, B, D = 40, 32, 2
    gi, whh, bhh, dhs = _scan_inputs('gru', T, B, D, H, 99 + H)
    h64, s64 = rr.gru_scan(gi, whh, bhh)
    g64 = rr.gru_scan_backward(dhs, whh, h64, s64)
    h32, s32 = rr.gru_scan(gi, whh, bhh, dtype=np.float32)
    g32 = rr.gru_scan_backward(dhs, whh, h32, s32, dtype=np.float32)
    hs, saved, dgi, dgh = _gru_launch(*_dev(gi, whh, bhh, dhs))
    split = lambda s: [s[..., k * H:(k + 1) * H] for k in range(4)]
    names = ['hs'] + ['saved.' + p for p in ('r', 'z', 'n', 'hn')] + ['dgi', 'dgh']
    _bounded('gru C ABI H=%d T=40 B=32 D=2' % H, names, [hs] + split(saved) + [dgi, dgh], [h32] + split(s32) + list(g32),
             [h64] + split(s64) + list(g64))


# ------------------------------------------------------------------------------------------------- e: inter-layer dropout
def _forward_of(which):
    from salsa_amd.crnn import fused_gru, fused_lstm
    return fused_gru.bigru_forward if which == 'bigru' else fused_lstm.rnn_forward


DROPOUT_CASES = [('bigru', 'gru', True), ('gru', 'gru', False), ('lstm', 'lstm', False), ('bilstm', 'lstm', True)]


def _masked_f32_cpu(rnn, x, gy, mask_tb):
    """the float32 yardstick with the mask: nn.GRU / nn.LSTM layer by layer in float32 on the CPU (two one-layer modules holding
    the two layers' parameters), the scaled mask between them -> [y, dx, every parameter gradient in rnn's parameter order]"""
    cls, D = type(rnn), 2 if rnn.bidirectional else 1
    sd = rnn.state_dict()
    mods = []
    for layer in range(rnn.num_layers):
        m = cls(rnn.input_size if layer == 0 else D * rnn.hidden_size, rnn.hidden_size, num_layers=1, batch_first=True,
                bidirectional=rnn.bidirectional)
        m.load_state_dict({k.replace('_l%d' % layer, '_l0'): v.clone() for k, v in sd.items() if '_l%d' % layer in k})
        mods.append(m)
    xr = x.clone().requires_grad_(True)
    h = mods[0](xr)[0]
    y = mods[1](h * mask_tb.transpose(0, 1))[0]
    y.backward(gy)
    grads = {}
    for layer, m in enumerate(mods):
        for k, p in m.named_parameters():
            grads[k.replace('_l0', '_l%d' % layer)] = p.grad
    return [y.detach(), xr.grad] + [grads[k] for k, _ in rnn.named_parameters()]


@pytest.mark.parametrize('decoder,kind,bidirectional', DROPOUT_CASES)
def test_inter_layer_dropout_is_placed_scaled_and_differentiated(decoder, kind, bidirectional, monkeypatch):
    """bigru_forward / rnn_forward on a two-layer module with dropout = 0.3, T = 40, B = 32, H = 256, F.dropout replaced by a
    recording function that applies a mask from a seeded generator.  In training: exactly one call, with the module's p, on the
    (T, B, D H) tensor that is layer 0's output; output and every gradient against the float64 reference with that mask.  With
    training=False, or dropout = 0.0: no call."""
    import torch.nn.functional as F
    T, B, H, p = 40, 32, 256, 0.3
    D = 2 if bidirectional else 1
    forward = _forward_of(decoder)
    rnn, x, gy = _rnn_case(kind, H, T, B, bidirectional, 110 + len(decoder), dropout=p)
    gen = torch.Generator().manual_seed(111)
    calls = []

    def recording_dropout(inp, p=0.5, training=True, inplace=False):
        keep = (torch.rand(inp.shape, generator=gen) >= p).float()
        calls.append(dict(x=inp.detach().clone(), p=p, training=training, keep=keep))
        return inp * keep.to(inp.device) / (1 - p)
    monkeypatch.setattr(F, 'dropout', recording_dropout)
    got, nodes = _run(rnn, x, gy, forward=forward)
    assert nodes.count('_LstmScanBackward' if kind == 'lstm' else '_GruScanBackward') == 2 and not [n for n in nodes if 'Rnn' in n], nodes
    assert len(calls) == rnn.num_layers - 1 == 1, len(calls)
    call = calls[0]
    assert call['p'] == rnn.dropout == p and call['training'] is True and tuple(call['x'].shape) == (T, B, D * H)
    # layer 0's output: what the same function returns for a one-layer module holding layer 0's parameters
    first = type(rnn)(512, H, num_layers=1, batch_first=True, bidirectional=bidirectional)
    first.load_state_dict({k: v for k, v in rnn.state_dict().items() if '_l0' in k})
    with torch.no_grad():
        out0 = forward(first.to(DEV), x.to(DEV), training=True)
    assert len(calls) == 1                                                    # (one layer: nothing to drop)
    assert torch.equal(call['x'], out0.transpose(0, 1)), 'the dropped tensor is not layer 0\'s output'
    mask = call['keep'].double().numpy() / (1 - p)                            # (T, B, D H), scaled
    params = {k: v.detach().double().numpy() for k, v in rnn.named_parameters()}
    y64, g64 = rr.rnn_forward_backward(kind, params, x.double().numpy(), gy.double().numpy(), 2, bidirectional, masks=[None, mask])
    ref = [y64, g64['input']] + [g64[k] for k, _ in rnn.named_parameters()]
    c32 = _masked_f32_cpu(rnn, x, gy, (call['keep'] / (1 - p)))
    _bounded('dropout %s T=%d B=%d H=%d' % (decoder, T, B, H), _names(rnn), got, c32, ref)
    # no dropout outside training, none with dropout = 0
    del calls[:]
    with torch.no_grad():
        forward(copy.deepcopy(rnn).to(DEV).eval(), x.to(DEV), training=False)
    assert calls == []
    rnn0, _, _ = _rnn_case(kind, H, T, B, bidirectional, 112, dropout=0.0)
    _run(rnn0, x, gy, forward=forward)
    assert calls == []


@pytest.mark.parametrize('decoder,kind,bidirectional', DROPOUT_CASES)
def test_real_dropout_masks_between_three_layers(decoder, kind, bidirectional, monkeypatch):
    """a three-layer module with the real F.dropout behind a recording pass-through: two calls, each output with 25 % - 35 % exact
    zeros (p = 0.3 over >= 1e5 elements: 5 points are > 30 standard deviations), the survivors its input times fl(1 / 0.7), the
    float32 product exactly; the two masks differ."""
    import torch.nn.functional as F
    T, B, H, p = 40, 32, 256, 0.3
    rnn, x, gy = _rnn_case(kind, H, T, B, bidirectional, 120 + len(decoder), dropout=p, layers=3)
    real, calls = F.dropout, []

    def passing_dropout(inp, p=0.5, training=True, inplace=False):
        out = real(inp, p=p, training=training, inplace=inplace)
        calls.append((inp.detach().clone(), out.detach().clone(), p, training))
        return out
    monkeypatch.setattr(F, 'dropout', passing_dropout)
    torch.manual_seed(121)
    got, nodes = _run(rnn, x, gy, forward=_forward_of(decoder))
    assert nodes.count('_LstmScanBackward' if kind == 'lstm' else '_GruScanBackward') == 3
    assert len(calls) == 2 and all(c[2] == p and c[3] is True for c in calls)
    scale = torch.tensor(1 / 0.7, dtype=torch.float32, device=DEV)
    zeros = []
    for inp, out, _, _ in calls:
        assert inp.numel() >= 10 ** 5 and tuple(inp.shape) == (T, B, (2 if bidirectional else 1) * H)
        dropped = out == 0
        frac = float(dropped.float().mean())
        _report('dropout %s three layers: zero fraction %.4f, |frac - 0.3| / 0.05' % (decoder, frac), abs(frac - 0.3) / 0.05)
        assert 0.25 <= frac <= 0.35, frac
        assert torch.equal(out[~dropped], (inp * scale)[~dropped])
        zeros.append(dropped)
    assert not torch.equal(zeros[0], zeros[1])
    assert all(bool(torch.isfinite(g).all()) for g in got)


# ------------------------------------------------------------------------------------------------- f: max / mean + max pools
POOL_MAPS = [(32, 512, 40, 12), (32, 512, 40, 8), (32, 512, 300, 12), (32, 512, 300, 8)]        # the frequency mean's list


def _guarded_like(shape, dtype, fill, pad):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * pad,), fill, dtype=dtype, device=DEV)
    return buf, buf[pad:pad + n].view(shape)


def _guards_hold(buf, view, fill, what):
    n, pad = view.numel(), (buf.numel() - view.numel()) // 2
    assert bool((buf[:pad] == fill).all()) and bool((buf[pad + n:] == fill).all()), what + ': a guard element changed'


@pytest.mark.parametrize('mode', ['max', 'avg_max'])
@pytest.mark.parametrize('shape', POOL_MAPS)
def test_freq_pool_kernels_at_bench_size(shape, mode):
    """salsa_nn_freq_pool_fwd / _bwd, both time_major values, on 'plain' and 'ties' input against rr.freq_pool /
    freq_pool_backward evaluated clip by clip.  The assertions of test_freq_pool_kernels_match_the_float64_reference: argmax equal
    everywhere (the lowest index holding the maximum), max exact, avg_max forward within rtol 1e-6 + atol 1e-6, backward exact
    for max and within one bf16 rounding (rtol 2^-6) for avg_max.  y, argmax and dx lie in pattern-filled guarded buffers."""
    N, Cn, H, W = shape
    L = _lib()
    m = {'max': 1, 'avg_max': 2}[mode]
    g = torch.Generator(device=DEV).manual_seed(130 + H + W)
    pad = 4 * Cn
    for kind in ('plain', 'ties'):
        x = _pool_input(N, Cn, H, W, g, kind)
        refs = [rr.freq_pool(x[n].float().cpu().numpy(), mode) for n in range(N)]             # per clip: (C, H) y and argmax
        if kind == 'ties':
            assert not bool(x[:, 0].any()) and bool((x[:, 1, :, W - 1] == x[:, 1, :, 0]).all())          # the ties are there
        for tm in (1, 0):
            rows = (H, N, Cn) if tm else (N, H, Cn)
            by, y = _guarded(rows, pad=pad)
            bam, am = _guarded_like(rows, torch.uint8, 0xA5, pad)
            with torch.cuda.device(DEV):
                assert L.salsa_nn_freq_pool_fwd(_p(x), _p(y), _p(am), N, H, W, Cn, m, tm, _stream()) == 0
            gy = torch.randn(rows, device=DEV, generator=g)
            bdx, dx = _guarded_like((N, H, W, Cn), torch.int16, 0x7FC1, pad)                  # bf16 NaN pattern; x's memory order
            with torch.cuda.device(DEV):
                assert L.salsa_nn_freq_pool_bwd(_p(gy), _p(am), _p(dx), N, H, W, Cn, m, tm, _stream()) == 0
            torch.cuda.synchronize()
            tag = 'freq pool %s %s tm=%d %dx%dx%dx%d' % (mode, kind, tm, N, Cn, H, W)
            _footprint(by, y, tag + ' y')
            _guards_hold(bam, am, 0xA5, tag + ' argmax')
            _guards_hold(bdx, dx, 0x7FC1, tag + ' dx')
            assert int(am.max()) < W, tag + ': an argmax was not written'
            dxf = dx.view(torch.bfloat16).permute(0, 3, 1, 2)                                  # (N, C, H, W) view
            assert bool(torch.isfinite(dxf.float()).all()), tag + ': a dx element was not written'
            clip = (lambda t, n: t[:, n]) if tm else (lambda t, n: t[n])                       # -> (H, C)
            worst = 0.0
            for n in range(N):
                ref_y, ref_am = refs[n]
                got_y, got_am = clip(y, n).cpu().numpy().T, clip(am, n).cpu().numpy().T.astype(np.int64)
                assert np.array_equal(got_am, ref_am), (tag, n)
                if mode == 'max':
                    assert np.array_equal(got_y, ref_y.astype(np.float32)), (tag, n)           # exact
                else:
                    np.testing.assert_allclose(got_y, ref_y, rtol=1e-6, atol=1e-6)
                    worst = max(worst, float((np.abs(got_y - ref_y) / (1e-6 + 1e-6 * np.abs(ref_y))).max()))
                g_ch = clip(gy, n).cpu().numpy().T.astype(np.float64)
                want = rr.freq_pool_backward(g_ch, ref_am, W, mode)
                want = torch.from_numpy(want).float().to(torch.bfloat16).float().numpy()
                got_dx = dxf[n].float().cpu().numpy()
                if mode == 'max':
                    assert np.array_equal(got_dx, want), (tag, n)
                else:
                    np.testing.assert_allclose(got_dx, want, rtol=2 ** -6, atol=1e-30)        # one bf16 rounding either way
            _report(tag + (' fwd' if mode == 'avg_max' else ' (exact)'), worst)
