"""Float64 numpy references for the decoder's Conformer blocks, independent of torch's implementation
(tests/test_conformer_cpu.py holds them against nn.LayerNorm, F.glu, nn.Conv1d, F.silu and the composed ConformerBlock): the three
kernel definitions of include/salsa_nn.h forward and backward, tensor for tensor, the whole block forward and backward, and the
counter-hash dropout mask restated from salsa_amd/csrc/nn_common.h / nn_batchnorm.hip.  Every function takes a dtype: every operand
is cast to it first, so dtype=np.float32 evaluates the same formulas in float32 -- the yardstick the GPU bounds are formed from.
A mask is a pair (keep, dropscale) or None (nothing dropped).

The formulas do not fix the order of their sums over channels and rows, and a float32 result depends on it.  By default they are
numpy's pairwise sums; inside `with sequential_sums():` they run left to right over the operand as given (a cumulative sum), the
plain loop's order, so that a permuted operand is summed in the permuted order."""
import contextlib

import numpy as np

import attn_reference as ar


# the mask seeds the GPU tests pass through the C ABI, and the torch.manual_seed from which their block test lets the product draw its
# six (tests/test_conformer_cpu.py checks on the CPU that each of them drops the quantised share)
GPU_TEST_SEEDS = (20211, 1234567891)
GPU_BLOCK_MANUAL_SEED = 31


_SEQUENTIAL = [False]


@contextlib.contextmanager
def sequential_sums():
    _SEQUENTIAL[0] = True
    try:
        yield
    finally:
        _SEQUENTIAL[0] = False


def _sum(a, axis, dtype, keepdims=False):
    if not _SEQUENTIAL[0]:
        return a.sum(axis=axis, keepdims=keepdims, dtype=dtype)
    t = np.take(np.cumsum(a, axis=axis, dtype=dtype), -1, axis=axis)
    return np.expand_dims(t, axis) if keepdims else t


def _mean(a, dtype):
    """over the last axis, kept"""
    return _sum(a, -1, dtype, keepdims=True) / dtype(a.shape[-1])


# ---- the dropout mask ---------------------------------------------------------------------------------------------------------------
def drop_threshold(p):
    """p quantised to 1 / 65536 as drop_args does it, in float32: (unsigned)(p * 65536.f + 0.5f), at most 65535; 0 for p <= 0"""
    if not p > 0:
        return 0
    return min(int(np.float32(p) * np.float32(65536.0) + np.float32(0.5)), 65535)


def drop_scale(p):
    """the float32 number kept elements are multiplied with: 65536.f / (float)(65536 - thresh)"""
    return np.float32(65536.0) / np.float32(65536 - drop_threshold(p))


def drop_hash(pair, seed):
    m = np.uint64(0xFFFFFFFF)
    h = (np.asarray(pair, np.uint64) * np.uint64(0x9E3779B1) + np.uint64(seed)) & m
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & m
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & m
    h ^= h >> np.uint64(16)
    return h


def drop_mask(shape, p, seed):
    """-> (keep, dropscale): element i of the flattened tensor takes 16 bits of the hash of (i >> 1, seed), the low half for even i,
    and is dropped when they are below the threshold"""
    n = int(np.prod(shape))
    idx = np.arange(n, dtype=np.uint64)
    h = drop_hash(idx >> np.uint64(1), seed)
    bits = np.where(idx & np.uint64(1), h >> np.uint64(16), h & np.uint64(0xFFFF))
    return (bits >= np.uint64(drop_threshold(p))).reshape(shape), drop_scale(p)


def _drop(v, mask, dtype):
    if mask is None:
        return v
    return np.where(mask[0], v * dtype(mask[1]), dtype(0))


# ---- pieces -------------------------------------------------------------------------------------------------------------------------
def sigmoid(v):
    return 1 / (1 + np.exp(-v))


def swish(v):
    return v * sigmoid(v)


def swish_grad(v):
    s = sigmoid(v)
    return s * (1 + v * (1 - s))


def layernorm_fwd(z, gamma, beta, eps=1e-5, dtype=np.float64):
    """-> y, mean, rstd over the last axis: biased variance, eps inside the square root, two-pass statistics"""
    z, gamma, beta = (np.asarray(a, dtype=dtype) for a in (z, gamma, beta))
    mean = _mean(z, dtype)
    var = _mean((z - mean) ** 2, dtype)
    rstd = dtype(1.0) / np.sqrt(var + dtype(eps))
    return ((z - mean) * rstd * gamma + beta).astype(dtype), mean[..., 0].astype(dtype), rstd[..., 0].astype(dtype)


def layernorm_bwd(dy, z, gamma, mean, rstd, dtype=np.float64):
    """-> dz, dgamma, dbeta"""
    dy, z, gamma, mean, rstd = (np.asarray(a, dtype=dtype) for a in (dy, z, gamma, mean, rstd))
    xhat = (z - mean[..., None]) * rstd[..., None]
    g = dy * gamma
    dz = rstd[..., None] * (g - _mean(g, dtype) - xhat * _mean(g * xhat, dtype))
    C = z.shape[-1]
    return dz.astype(dtype), _sum((dy * xhat).reshape(-1, C), 0, dtype), _sum(dy.reshape(-1, C), 0, dtype)


# ---- salsa_nn_res_layernorm ---------------------------------------------------------------------------------------------------------
def res_z(x, branch, scale, mask, dtype=np.float64):
    x = np.asarray(x, dtype=dtype)
    if branch is None:
        return x
    t = x + dtype(scale) * (np.asarray(branch, dtype=dtype) * dtype(1.0 if mask is None else mask[1]))
    return t if mask is None else np.where(mask[0], t, x)


def res_layernorm_fwd(x, branch, scale, mask, gamma, beta, eps=1e-5, dtype=np.float64):
    """z = x + scale * drop(branch) (branch None: x), y = LayerNorm(z) gamma + beta -> z, y, mean, rstd"""
    z = res_z(x, branch, scale, mask, dtype)
    return (z,) + layernorm_fwd(z, gamma, beta, eps, dtype)


def res_layernorm_bwd(dy, dz_in, x, branch, scale, mask, gamma, mean, rstd, dtype=np.float64):
    """-> dx = dz_in + LayerNorm_backward(dy), dbranch = scale mask dropscale dx (None without a branch), dgamma, dbeta (None
    without dy)"""
    z = res_z(x, branch, scale, mask, dtype)
    dx, dgamma, dbeta = np.zeros_like(z), None, None
    if dy is not None:
        dx, dgamma, dbeta = layernorm_bwd(dy, z, gamma, mean, rstd, dtype)
    if dz_in is not None:
        dx = np.asarray(dz_in, dtype=dtype) + dx
    dbranch = None
    if branch is not None:
        dbranch = dtype(scale) * (dx * dtype(1.0 if mask is None else mask[1]))
        if mask is not None:
            dbranch = np.where(mask[0], dbranch, dtype(0))
    return dx.astype(dtype), dbranch, dgamma, dbeta


# ---- salsa_nn_bias_swish_dropout ----------------------------------------------------------------------------------------------------
def bias_swish_dropout_fwd(a, bias, mask, dtype=np.float64):
    a, bias = np.asarray(a, dtype=dtype), np.asarray(bias, dtype=dtype)
    return _drop(swish(a + bias), mask, dtype).astype(dtype)


def bias_swish_dropout_bwd(dh, a, bias, mask, dtype=np.float64):
    """-> da, dbias (the column sum of da)"""
    dh, a, bias = (np.asarray(t, dtype=dtype) for t in (dh, a, bias))
    da = (_drop(dh, mask, dtype) * swish_grad(a + bias)).astype(dtype)
    return da, _sum(da.reshape(-1, a.shape[-1]), 0, dtype)


# ---- salsa_nn_conv_module -----------------------------------------------------------------------------------------------------------
def _taps(K, reverse):
    return range(K - 1, -1, -1) if reverse else range(K)


def conv_module_parts(a, w, wb, gamma, beta, eps, dtype, reverse=False):
    a, w, wb = np.asarray(a, dtype=dtype), np.asarray(w, dtype=dtype), np.asarray(wb, dtype=dtype)
    B, T, d2 = a.shape
    d, K = d2 // 2, w.shape[1]
    s = sigmoid(a[..., d:])
    pad = np.zeros((B, T + K - 1, d), dtype=dtype)                           # zero rows before 0 and from T on, per sample
    pad[:, K // 2:K // 2 + T] = a[..., :d] * s
    v = np.broadcast_to(wb, (B, T, d)).astype(dtype)
    for k in _taps(K, reverse):
        v = v + w[:, k] * pad[:, k:k + T]
    y, mean, rstd = layernorm_fwd(v, gamma, beta, eps, dtype)
    return s, pad, v, y, mean, rstd


def conv_module_fwd(a, w, wb, gamma, beta, eps=1e-5, dtype=np.float64, reverse=False):
    """u = swish(LayerNorm(DW(glu(a))) gamma + beta): a (B, T, 2 d), w (d, K), -> u (B, T, d); reverse: the taps summed from the last"""
    return swish(conv_module_parts(a, w, wb, gamma, beta, eps, dtype, reverse)[3]).astype(dtype)


def conv_module_bwd(du, a, w, wb, gamma, beta, eps=1e-5, dtype=np.float64, reverse=False):
    """-> da (B, T, 2 d), dw (d, K), dwb, dgamma, dbeta (d,)"""
    s, pad, v, y, mean, rstd = conv_module_parts(a, w, wb, gamma, beta, eps, dtype, reverse)
    a, w, du = np.asarray(a, dtype=dtype), np.asarray(w, dtype=dtype), np.asarray(du, dtype=dtype)
    B, T, d2 = a.shape
    d, K = d2 // 2, w.shape[1]
    dv, dgamma, dbeta = layernorm_bwd(du * swish_grad(y), v, gamma, mean, rstd, dtype)
    dw = np.stack([_sum((dv * pad[:, k:k + T]).reshape(-1, d), 0, dtype) for k in range(K)], axis=1)
    dvp = np.zeros((B, T + K - 1, d), dtype=dtype)
    dvp[:, K // 2:K // 2 + T] = dv
    dgl = np.zeros((B, T, d), dtype=dtype)
    for k in _taps(K, reverse):                                              # dglu[t] = sum_k w[k] dv[t + K/2 - k]
        dgl = dgl + w[:, k] * dvp[:, K - 1 - k:K - 1 - k + T]
    da = np.concatenate([dgl * s, dgl * a[..., :d] * s * (1 - s)], axis=-1)
    return da.astype(dtype), dw.astype(dtype), _sum(dv.reshape(-1, d), 0, dtype), dgamma, dbeta


# ---- the whole block ----------------------------------------------------------------------------------------------------------------
SITES = ('ff1_in', 'ff1', 'att', 'conv', 'ff2_in', 'ff2')                     # the dropout sites, in the order their seeds are drawn


def _lin_bwd(dout, n, W):
    d2, n2 = dout.reshape(-1, dout.shape[-1]), n.reshape(-1, n.shape[-1])
    return dout @ W, d2.T @ n2, d2.sum(axis=0)


def block(x, P, n_heads, eps=1e-5, masks=None, dy=None, dtype=np.float64):
    """One ConformerBlock.  P: its state dict as numpy arrays; masks: {site: (keep, dropscale)} (missing / None: no dropout there).
    -> y, or with dy: (y, dx, {key: gradient})."""
    masks = masks or {}
    P = {k: np.asarray(v, dtype=dtype) for k, v in P.items()}
    x = np.asarray(x, dtype=dtype)
    B, T, d = x.shape
    wdw = P['conv_dw.weight'].reshape(d, -1)

    def norm(name):
        return P[name + '.weight'], P[name + '.bias']

    def ff_fwd(n, pre, site):
        a = n @ P[pre + '_w1.weight'].T
        h = bias_swish_dropout_fwd(a, P[pre + '_w1.bias'], masks.get(site), dtype)
        return h @ P[pre + '_w2.weight'].T + P[pre + '_w2.bias'], (n, a, h)

    def ff_bwd(df, pre, site, cache, G):
        n, a, h = cache
        dh, G[pre + '_w2.weight'], G[pre + '_w2.bias'] = _lin_bwd(df, h, P[pre + '_w2.weight'])
        da, G[pre + '_w1.bias'] = bias_swish_dropout_bwd(dh, a, P[pre + '_w1.bias'], masks.get(site), dtype)
        dn, G[pre + '_w1.weight'], _ = _lin_bwd(da, n, P[pre + '_w1.weight'])
        return dn

    _, n1, mu1, rs1 = res_layernorm_fwd(x, None, 1.0, None, *norm('norm_ff1'), eps, dtype)
    f1, c_ff1 = ff_fwd(n1, 'ff1', 'ff1_in')
    x1, n2, mu2, rs2 = res_layernorm_fwd(x, f1, 0.5, masks.get('ff1'), *norm('norm_att'), eps, dtype)
    qkv = (n2 @ P['mha.in_proj_weight'].T + P['mha.in_proj_bias']).reshape(B, T, 3, n_heads, d // n_heads)
    o, lse = ar.attn_core_fwd(qkv, dtype)
    at = o @ P['mha.out_proj.weight'].T + P['mha.out_proj.bias']
    x2, n3, mu3, rs3 = res_layernorm_fwd(x1, at, 1.0, masks.get('att'), *norm('norm_conv'), eps, dtype)
    ca = n3 @ P['conv_p1.weight'].T + P['conv_p1.bias']
    cv = (ca, wdw, P['conv_dw.bias'], *norm('conv_norm'), eps, dtype)
    u = conv_module_fwd(*cv)
    c = u @ P['conv_p2.weight'].T + P['conv_p2.bias']
    x3, n4, mu4, rs4 = res_layernorm_fwd(x2, c, 1.0, masks.get('conv'), *norm('norm_ff2'), eps, dtype)
    f2, c_ff2 = ff_fwd(n4, 'ff2', 'ff2_in')
    _, y, mu5, rs5 = res_layernorm_fwd(x3, f2, 0.5, masks.get('ff2'), *norm('norm_out'), eps, dtype)
    if dy is None:
        return y
    G = {}
    dy = np.asarray(dy, dtype=dtype)
    dx3, df2, G['norm_out.weight'], G['norm_out.bias'] = res_layernorm_bwd(dy, None, x3, f2, 0.5, masks.get('ff2'), P['norm_out.weight'], mu5, rs5, dtype)
    dn4 = ff_bwd(df2, 'ff2', 'ff2_in', c_ff2, G)
    dx2, dc, G['norm_ff2.weight'], G['norm_ff2.bias'] = res_layernorm_bwd(dn4, dx3, x2, c, 1.0, masks.get('conv'), P['norm_ff2.weight'], mu4, rs4, dtype)
    du, G['conv_p2.weight'], G['conv_p2.bias'] = _lin_bwd(dc, u, P['conv_p2.weight'])
    dca, dwdw, G['conv_dw.bias'], G['conv_norm.weight'], G['conv_norm.bias'] = conv_module_bwd(du, *cv)
    G['conv_dw.weight'] = dwdw.reshape(P['conv_dw.weight'].shape)
    dn3, G['conv_p1.weight'], G['conv_p1.bias'] = _lin_bwd(dca, n3, P['conv_p1.weight'])
    dx1, dat, G['norm_conv.weight'], G['norm_conv.bias'] = res_layernorm_bwd(dn3, dx2, x1, at, 1.0, masks.get('att'), P['norm_conv.weight'], mu3, rs3, dtype)
    do, G['mha.out_proj.weight'], G['mha.out_proj.bias'] = _lin_bwd(dat, o, P['mha.out_proj.weight'])
    dqkv = ar.attn_core_bwd(qkv, o, lse, do, dtype).reshape(B, T, 3 * d)
    dn2, G['mha.in_proj_weight'], G['mha.in_proj_bias'] = _lin_bwd(dqkv, n2, P['mha.in_proj_weight'])
    dx0, df1, G['norm_att.weight'], G['norm_att.bias'] = res_layernorm_bwd(dn2, dx1, x, f1, 0.5, masks.get('ff1'), P['norm_att.weight'], mu2, rs2, dtype)
    dn1 = ff_bwd(df1, 'ff1', 'ff1_in', c_ff1, G)
    dx, _, G['norm_ff1.weight'], G['norm_ff1.bias'] = res_layernorm_bwd(dn1, dx0, x, None, 1.0, None, P['norm_ff1.weight'], mu1, rs1, dtype)
    return y, dx, G
