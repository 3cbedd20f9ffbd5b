"""Float64 numpy references for the decoder's self-attention stage, independent of torch's implementation
(tests/test_attn_cpu.py holds them against nn.MultiheadAttention and nn.LayerNorm): the attention core on the packed
(B, T, 3, heads, dh) in-projection output, forward with lse and backward, and the residual add + LayerNorm, forward and backward.
They mirror the C ABI of include/salsa_nn.h tensor for tensor.  Every function takes a dtype: every operand is cast to it first, so
dtype=np.float32 evaluates the same formulas in float32 -- the yardstick the GPU bounds are formed from."""
import numpy as np


def attn_core_fwd(qkv, dtype=np.float64):
    """qkv (B, T, 3, heads, dh) -> out (B, T, heads * dh), lse (B, heads, T)"""
    qkv = np.asarray(qkv, dtype=dtype)
    B, T, _, H, dh = qkv.shape
    q, k, v = (qkv[:, :, i].transpose(0, 2, 1, 3) for i in range(3))                 # (B, H, T, dh)
    s = np.matmul(q, k.transpose(0, 1, 3, 2)) * dtype(1.0 / np.sqrt(dh))             # (B, H, T, T)
    m = s.max(axis=-1, keepdims=True)
    p = np.exp(s - m)
    l = p.sum(axis=-1, keepdims=True)
    out = np.matmul(p, v) / l
    lse = (m + np.log(l))[..., 0]
    return out.transpose(0, 2, 1, 3).reshape(B, T, H * dh).astype(dtype), lse.astype(dtype)


def attn_core_bwd(qkv, out, lse, d_out, dtype=np.float64):
    """-> d_qkv (B, T, 3, heads, dh): P recomputed from lse, delta = rowsum(d_out * out), as the kernel's statement"""
    qkv, out, lse, d_out = (np.asarray(a, dtype=dtype) for a in (qkv, out, lse, d_out))
    B, T, _, H, dh = qkv.shape
    scale = dtype(1.0 / np.sqrt(dh))
    q, k, v = (qkv[:, :, i].transpose(0, 2, 1, 3) for i in range(3))
    o = out.reshape(B, T, H, dh).transpose(0, 2, 1, 3)
    g = d_out.reshape(B, T, H, dh).transpose(0, 2, 1, 3)
    p = np.exp(np.matmul(q, k.transpose(0, 1, 3, 2)) * scale - lse[..., None])
    delta = (g * o).sum(axis=-1, keepdims=True)
    ds = p * (np.matmul(g, v.transpose(0, 1, 3, 2)) - delta)
    dq = np.matmul(ds, k) * scale
    dk = np.matmul(ds.transpose(0, 1, 3, 2), q) * scale
    dv = np.matmul(p.transpose(0, 1, 3, 2), g)
    return np.stack([t.transpose(0, 2, 1, 3) for t in (dq, dk, dv)], axis=2).astype(dtype)


def add_layernorm_fwd(x, res, gamma, beta, eps=1e-5, dtype=np.float64):
    """-> y (M, C), mean (M,), rstd (M,): biased variance, eps inside the square root, two-pass statistics"""
    x, res, gamma, beta = (np.asarray(a, dtype=dtype) for a in (x, res, gamma, beta))
    z = x + res
    mean = z.mean(axis=-1, keepdims=True, dtype=dtype)
    var = ((z - mean) ** 2).mean(axis=-1, keepdims=True, dtype=dtype)
    rstd = dtype(1.0) / np.sqrt(var + dtype(eps))
    y = (z - mean) * rstd * gamma + beta
    return y.astype(dtype), mean[..., 0].astype(dtype), rstd[..., 0].astype(dtype)


def add_layernorm_bwd(dy, x, res, gamma, mean, rstd, dtype=np.float64):
    """-> dx (M, C) (the gradient of x and of res), dgamma (C,), dbeta (C,)"""
    dy, x, res, gamma, mean, rstd = (np.asarray(a, dtype=dtype) for a in (dy, x, res, gamma, mean, rstd))
    xhat = (x + res - mean[..., None]) * rstd[..., None]
    g = dy * gamma
    dx = rstd[..., None] * (g - g.mean(axis=-1, keepdims=True, dtype=dtype) - xhat * (g * xhat).mean(axis=-1, keepdims=True, dtype=dtype))
    C = x.shape[-1]
    return dx.astype(dtype), (dy * xhat).reshape(-1, C).sum(axis=0, dtype=dtype), dy.reshape(-1, C).sum(axis=0, dtype=dtype)


def block_fwd(x, in_w, in_b, out_w, out_b, gamma, beta, n_heads, eps=1e-5, dtype=np.float64):
    """one AttnBlock without dropout: LayerNorm(x + out_proj(attn_core(in_proj(x)))); x (B, T, d)"""
    x, in_w, in_b, out_w, out_b = (np.asarray(a, dtype=dtype) for a in (x, in_w, in_b, out_w, out_b))
    B, T, d = x.shape
    qkv = (x @ in_w.T + in_b).reshape(B, T, 3, n_heads, d // n_heads)
    a, _ = attn_core_fwd(qkv, dtype)
    return add_layernorm_fwd(a @ out_w.T + out_b, x, gamma, beta, eps, dtype)[0]
