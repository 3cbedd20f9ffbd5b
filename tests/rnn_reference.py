"""Float64 numpy references for the decoder options: LSTM and GRU layers (forward and BPTT, gate orders i,f,g,o and r,z,n as in
torch.nn) and the frequency max / mean + max pools with the kernels' tie rule (the LOWEST index holding the maximum; the first
NaN wins).  Independent of torch's implementation: tests/test_crnn_decoders_cpu.py holds them against nn.LSTM / nn.GRU.  The
layer functions take a dtype (float32: the same formulas as a float32 yardstick); lstm_scan / gru_scan and their backwards mirror
the C ABI of include/salsa_gru.h tensor for tensor; rnn_forward_backward takes inter-layer dropout masks."""
import numpy as np


def _sig(x):
    with np.errstate(over='ignore'):                  # exp(-x) = inf for x < -709 (float32: < -88.7): the gate is then exactly 0
        return 1.0 / (1.0 + np.exp(-x))


def _steps(T, reverse):
    return range(T - 1, -1, -1) if reverse else range(T)


def lstm_layer(x, wih, whh, bih, bhh, reverse=False, dtype=np.float64):
    """x (T, B, In) -> (hs (T, B, H), cache); one direction; the scan runs t = T-1..0 when reverse and stores at index t.  Every
    operand is cast to dtype first, so dtype=np.float32 evaluates the same formulas in float32."""
    x, wih, whh, bih, bhh = (np.asarray(a, dtype=dtype) for a in (x, wih, whh, bih, bhh))
    T, B, _ = x.shape
    H = whh.shape[1]
    h, c = np.zeros((B, H), dtype), np.zeros((B, H), dtype)
    hs, cache = np.zeros((T, B, H), dtype), [None] * T
    for t in _steps(T, reverse):
        a = x[t] @ wih.T + bih + h @ whh.T + bhh
        i, f, g, o = _sig(a[:, :H]), _sig(a[:, H:2 * H]), np.tanh(a[:, 2 * H:3 * H]), _sig(a[:, 3 * H:])
        cache[t] = (h, c, i, f, g, o)
        c = f * c + i * g
        h = o * np.tanh(c)
        hs[t] = h
        cache[t] = cache[t] + (c,)
    return hs, cache


def lstm_layer_backward(x, wih, whh, dhs, cache, reverse=False, dtype=np.float64):
    """-> dx, dwih, dwhh, dbih, dbhh for the layer of lstm_layer"""
    x, wih, whh, dhs = (np.asarray(a, dtype=dtype) for a in (x, wih, whh, dhs))
    T, B, _ = x.shape
    H = whh.shape[1]
    dx = np.zeros_like(x)
    dwih, dwhh, db = np.zeros_like(wih), np.zeros_like(whh), np.zeros(4 * H, dtype)
    dh, dc = np.zeros((B, H), dtype), np.zeros((B, H), dtype)
    for t in _steps(T, not reverse):
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


def gru_layer(x, wih, whh, bih, bhh, reverse=False, dtype=np.float64):
    x, wih, whh, bih, bhh = (np.asarray(a, dtype=dtype) for a in (x, wih, whh, bih, bhh))
    T, B, _ = x.shape
    H = whh.shape[1]
    h = np.zeros((B, H), dtype)
    hs, cache = np.zeros((T, B, H), dtype), [None] * T
    for t in _steps(T, reverse):
        gx, gh = x[t] @ wih.T + bih, h @ whh.T + bhh
        r = _sig(gx[:, :H] + gh[:, :H])
        z = _sig(gx[:, H:2 * H] + gh[:, H:2 * H])
        n = np.tanh(gx[:, 2 * H:] + r * gh[:, 2 * H:])
        cache[t] = (h, r, z, n, gh[:, 2 * H:])
        h = (1 - z) * n + z * h
        hs[t] = h
    return hs, cache


def gru_layer_backward(x, wih, whh, dhs, cache, reverse=False, dtype=np.float64):
    x, wih, whh, dhs = (np.asarray(a, dtype=dtype) for a in (x, wih, whh, dhs))
    T, B, _ = x.shape
    H = whh.shape[1]
    dx = np.zeros_like(x)
    dwih, dwhh, dbih, dbhh = np.zeros_like(wih), np.zeros_like(whh), np.zeros(3 * H, dtype), np.zeros(3 * H, dtype)
    dh = np.zeros((B, H), dtype)
    for t in _steps(T, not reverse):
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


# ---------------------------------------------------------------------------------------------- the scans at the C ABI
# The tensors of include/salsa_gru.h, axis for axis: direction d = 1 scans t = T-1..0 and stores at index t.  Written apart from
# the layer functions above (tests/test_crnn_decoders_cpu.py holds the two against each other).
def lstm_scan(gi, whh, bhh, dtype=np.float64):
    """gi [T][B][D][4H] (W_ih x + b_ih), whh [D][4H][H], bhh [D][4H] -> hs [T][B][D][H], saved [T][B][D][5H] = i, f, g, o
    (activated) and c after the step"""
    gi, whh, bhh = (np.asarray(a, dtype=dtype) for a in (gi, whh, bhh))
    T, B, D, H4 = gi.shape
    H = H4 // 4
    hs, saved = np.zeros((T, B, D, H), dtype), np.zeros((T, B, D, 5 * H), dtype)
    for d in range(D):
        wt = np.ascontiguousarray(whh[d].T)
        h, c = np.zeros((B, H), dtype), np.zeros((B, H), dtype)
        for t in _steps(T, d == 1):
            a = gi[t, :, d] + (h @ wt + bhh[d])
            sv = saved[t, :, d]
            sv[:, :H], sv[:, H:2 * H], sv[:, 3 * H:4 * H] = _sig(a[:, :H]), _sig(a[:, H:2 * H]), _sig(a[:, 3 * H:])
            sv[:, 2 * H:3 * H] = np.tanh(a[:, 2 * H:3 * H])
            c = sv[:, H:2 * H] * c + sv[:, :H] * sv[:, 2 * H:3 * H]
            h = sv[:, 3 * H:4 * H] * np.tanh(c)
            sv[:, 4 * H:] = c
            hs[t, :, d] = h
    return hs, saved


def lstm_scan_backward(dhs, whh, saved, dtype=np.float64):
    """dhs [T][B][D][H], whh [D][4H][H], saved of lstm_scan -> dg [T][B][D][4H], the gradient wrt the gate pre-activations"""
    dhs, whh, saved = (np.asarray(a, dtype=dtype) for a in (dhs, whh, saved))
    T, B, D, H = dhs.shape
    dg = np.zeros((T, B, D, 4 * H), dtype)
    for d in range(D):
        dh, dc = np.zeros((B, H), dtype), np.zeros((B, H), dtype)
        order = list(_steps(T, d == 1))
        for s in range(T - 1, -1, -1):
            t = order[s]
            i, f, g, o, c = (saved[t, :, d, k * H:(k + 1) * H] for k in range(5))
            cp = saved[order[s - 1], :, d, 4 * H:] if s > 0 else np.zeros((B, H), dtype)
            dh = dh + dhs[t, :, d]
            tc = np.tanh(c)
            dc = dc + dh * o * (1 - tc * tc)
            out = dg[t, :, d]
            out[:, :H], out[:, H:2 * H] = dc * g * i * (1 - i), dc * cp * f * (1 - f)
            out[:, 2 * H:3 * H], out[:, 3 * H:] = dc * i * (1 - g * g), dh * tc * o * (1 - o)
            dh = out @ whh[d]
            dc = dc * f
    return dg


def gru_scan(gi, whh, bhh, dtype=np.float64):
    """gi [T][B][D][3H], whh [D][3H][H], bhh [D][3H] -> hs [T][B][D][H], saved [T][B][D][4H] = r, z, n, W_hn h + b_hn"""
    gi, whh, bhh = (np.asarray(a, dtype=dtype) for a in (gi, whh, bhh))
    T, B, D, H3 = gi.shape
    H = H3 // 3
    hs, saved = np.zeros((T, B, D, H), dtype), np.zeros((T, B, D, 4 * H), dtype)
    for d in range(D):
        wt = np.ascontiguousarray(whh[d].T)
        h = np.zeros((B, H), dtype)
        for t in _steps(T, d == 1):
            gh = h @ wt + bhh[d]
            g, sv = gi[t, :, d], saved[t, :, d]
            sv[:, :H] = _sig(g[:, :H] + gh[:, :H])
            sv[:, H:2 * H] = _sig(g[:, H:2 * H] + gh[:, H:2 * H])
            sv[:, 3 * H:] = gh[:, 2 * H:]
            sv[:, 2 * H:3 * H] = np.tanh(g[:, 2 * H:] + sv[:, :H] * gh[:, 2 * H:])
            h = (1 - sv[:, H:2 * H]) * sv[:, 2 * H:3 * H] + sv[:, H:2 * H] * h
            hs[t, :, d] = h
    return hs, saved


def gru_scan_backward(dhs, whh, hs, saved, dtype=np.float64):
    """-> dgi [T][B][D][3H] (gradient wrt gi) and dgh [T][B][D][3H] (gradient wrt W_hh h_prev + b_hh)"""
    dhs, whh, hs, saved = (np.asarray(a, dtype=dtype) for a in (dhs, whh, hs, saved))
    T, B, D, H = dhs.shape
    dgi, dgh = np.zeros((T, B, D, 3 * H), dtype), np.zeros((T, B, D, 3 * H), dtype)
    for d in range(D):
        dh = np.zeros((B, H), dtype)
        order = list(_steps(T, d == 1))
        for s in range(T - 1, -1, -1):
            t = order[s]
            r, z, n, hn = (saved[t, :, d, k * H:(k + 1) * H] for k in range(4))
            hp = hs[order[s - 1], :, d] if s > 0 else np.zeros((B, H), dtype)
            dh = dh + dhs[t, :, d]
            dn = dh * (1 - z) * (1 - n * n)
            dz = dh * (hp - n) * z * (1 - z)
            dr = dn * hn * r * (1 - r)
            dgi[t, :, d] = np.concatenate([dr, dz, dn], axis=1)
            dgh[t, :, d] = np.concatenate([dr, dz, dn * r], axis=1)
            dh = dgh[t, :, d] @ whh[d] + dh * z
    return dgi, dgh


def rnn_forward_backward(kind, params, x, dy, num_layers, bidirectional, masks=None):
    """A batch_first multi-layer (bi)LSTM / GRU in float64: params {torch parameter name: ndarray}, x (B, T, In),
    dy (B, T, D*H) -> (y (B, T, D*H), {'input': dx, name: gradient}).  Inter-layer dropout with given masks: masks[l]
    (T, B, D*H), already scaled by 1 / (1 - p), multiplies the input of layer l >= 1 in the forward and the gradient flowing back
    out of it (masks[0] is not read; masks=None or masks[l] None: no dropout)."""
    layer_f, back_f = (lstm_layer, lstm_layer_backward) if kind == 'lstm' else (gru_layer, gru_layer_backward)
    sfx = ('', '_reverse') if bidirectional else ('',)
    mask = lambda l: None if (masks is None or l == 0 or masks[l] is None) else np.asarray(masks[l], dtype=np.float64)
    inp, caches = [np.transpose(x, (1, 0, 2)).astype(np.float64)], []
    for layer in range(num_layers):
        if mask(layer) is not None:
            inp[-1] = inp[-1] * mask(layer)                       # the layer's input as it consumed it
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
        dout = dinp if mask(layer) is None else dinp * mask(layer)
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
