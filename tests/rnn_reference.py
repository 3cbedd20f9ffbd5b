"""Float64 numpy references for the decoder options: LSTM and GRU layers (forward and BPTT, gate orders i,f,g,o and r,z,n as in
torch.nn) and the frequency max / mean + max pools with the kernels' tie rule (the LOWEST index holding the maximum; the first
NaN wins).  Independent of torch's implementation: tests/test_crnn_decoders_cpu.py holds them against nn.LSTM / nn.GRU."""
import numpy as np


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def lstm_layer(x, wih, whh, bih, bhh, reverse=False):
    """x (T, B, In) -> (hs (T, B, H), cache); one direction; the scan runs t = T-1..0 when reverse and stores at index t"""
    T, B, _ = x.shape
    H = whh.shape[1]
    h, c = np.zeros((B, H)), np.zeros((B, H))
    hs, cache = np.zeros((T, B, H)), [None] * T
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        a = x[t] @ wih.T + bih + h @ whh.T + bhh
        i, f, g, o = _sig(a[:, :H]), _sig(a[:, H:2 * H]), np.tanh(a[:, 2 * H:3 * H]), _sig(a[:, 3 * H:])
        cache[t] = (h, c, i, f, g, o)
        c = f * c + i * g
        h = o * np.tanh(c)
        hs[t] = h
        cache[t] = cache[t] + (c,)
    return hs, cache


def lstm_layer_backward(x, wih, whh, dhs, cache, reverse=False):
    """-> dx, dwih, dwhh, dbih, dbhh for the layer of lstm_layer"""
    T, B, _ = x.shape
    H = whh.shape[1]
    dx = np.zeros_like(x)
    dwih, dwhh, db = np.zeros_like(wih), np.zeros_like(whh), np.zeros(4 * H)
    dh, dc = np.zeros((B, H)), np.zeros((B, H))
    for t in (range(T) if reverse else range(T - 1, -1, -1)):
        hp, cp, i, f, g, o, c = cache[t]
        dh = dh + dhs[t]
        tc = np.tanh(c)
        dc = dc + dh * o * (1 - tc * tc)
        da = np.concatenate([dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], axis=1)
        dx[t] = da @ wih
        dwih += da.T @ x[t]
        dwhh += da.T @ hp
        db += da.sum(0)
        dh = da @ whh
        dc = dc * f
    return dx, dwih, dwhh, db, db.copy()


def gru_layer(x, wih, whh, bih, bhh, reverse=False):
    T, B, _ = x.shape
    H = whh.shape[1]
    h = np.zeros((B, H))
    hs, cache = np.zeros((T, B, H)), [None] * T
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        gx, gh = x[t] @ wih.T + bih, h @ whh.T + bhh
        r = _sig(gx[:, :H] + gh[:, :H])
        z = _sig(gx[:, H:2 * H] + gh[:, H:2 * H])
        n = np.tanh(gx[:, 2 * H:] + r * gh[:, 2 * H:])
        cache[t] = (h, r, z, n, gh[:, 2 * H:])
        h = (1 - z) * n + z * h
        hs[t] = h
    return hs, cache


def gru_layer_backward(x, wih, whh, dhs, cache, reverse=False):
    T, B, _ = x.shape
    H = whh.shape[1]
    dx = np.zeros_like(x)
    dwih, dwhh, dbih, dbhh = np.zeros_like(wih), np.zeros_like(whh), np.zeros(3 * H), np.zeros(3 * H)
    dh = np.zeros((B, H))
    for t in (range(T) if reverse else range(T - 1, -1, -1)):
        hp, r, z, n, hn = cache[t]
        dh = dh + dhs[t]
        dn = dh * (1 - z) * (1 - n * n)
        dz = dh * (hp - n) * z * (1 - z)
        dr = dn * hn * r * (1 - r)
        dgx = np.concatenate([dr, dz, dn], axis=1)
        dgh = np.concatenate([dr, dz, dn * r], axis=1)
        dx[t] = dgx @ wih
        dwih += dgx.T @ x[t]
        dwhh += dgh.T @ hp
        dbih += dgx.sum(0)
        dbhh += dgh.sum(0)
        dh = dgh @ whh + dh * z
    return dx, dwih, dwhh, dbih, dbhh


def rnn_forward_backward(kind, params, x, dy, num_layers, bidirectional):
    """A batch_first multi-layer (bi)LSTM / GRU without dropout in float64: params {torch parameter name: ndarray}, x (B, T, In),
    dy (B, T, D*H) -> (y (B, T, D*H), {'input': dx, name: gradient})"""
    layer_f, back_f = (lstm_layer, lstm_layer_backward) if kind == 'lstm' else (gru_layer, gru_layer_backward)
    sfx = ('', '_reverse') if bidirectional else ('',)
    inp, caches = [np.transpose(x, (1, 0, 2)).astype(np.float64)], []
    for layer in range(num_layers):
        outs, cs = [], []
        for d, s in enumerate(sfx):
            p = [params['%s_l%d%s' % (k, layer, s)] for k in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]
            hs, cache = layer_f(inp[-1], *p, reverse=d == 1)
            outs.append(hs)
            cs.append(cache)
        inp.append(np.concatenate(outs, axis=2))
        caches.append(cs)
    y = np.transpose(inp[-1], (1, 0, 2))
    grads, dout = {}, np.transpose(dy, (1, 0, 2)).astype(np.float64)
    for layer in range(num_layers - 1, -1, -1):
        H = params['weight_hh_l%d' % layer].shape[1]
        dinp = np.zeros_like(inp[layer])
        for d, s in enumerate(sfx):
            wih, whh = params['weight_ih_l%d%s' % (layer, s)], params['weight_hh_l%d%s' % (layer, s)]
            dx, dwih, dwhh, dbih, dbhh = back_f(inp[layer], wih, whh, dout[:, :, d * H:(d + 1) * H], caches[layer][d], reverse=d == 1)
            dinp += dx
            for k, v in (('weight_ih', dwih), ('weight_hh', dwhh), ('bias_ih', dbih), ('bias_hh', dbhh)):
                grads['%s_l%d%s' % (k, layer, s)] = v
        dout = dinp
    grads['input'] = np.transpose(dout, (1, 0, 2))
    return y, grads


def freq_pool(x, mode):
    """x (..., W) -> (y, argmax) over the last axis in float64: mode 'max' or 'avg_max' (mean + max); argmax is the lowest index
    holding the maximum, or the first NaN's index when there is one (y is then NaN)"""
    x = np.asarray(x, dtype=np.float64)
    nan = np.isnan(x)
    first_nan = np.argmax(nan, axis=-1)
    am = np.where(nan.any(-1), first_nan, np.argmax(np.where(nan, -np.inf, x), axis=-1))   # np.argmax: the first occurrence
    mx = np.take_along_axis(x, am[..., None], axis=-1)[..., 0]
    return (mx if mode == 'max' else x.mean(-1) + mx), am


def freq_pool_backward(g, am, W, mode):
    """g (...) -> dx (..., W): g / W (avg_max) + g at the argmax"""
    dx = np.zeros(g.shape + (W,))
    np.put_along_axis(dx, am[..., None], np.asarray(g, dtype=np.float64)[..., None], axis=-1)
    if mode == 'avg_max':
        dx += np.asarray(g, dtype=np.float64)[..., None] / W
    return dx
