"""The decoder's optional self-attention stage: y = LayerNorm(x + dropout(MHSA(x))) per block, after the
recurrent stack.  The parameters live in plain torch modules (AttnBlock in model.py: nn.MultiheadAttention, nn.LayerNorm,
nn.Dropout), so their initialisation, state-dict keys and the CPU path are torch's own.  On the GPU the two projections stay GEMMs
and the rest runs on two hand-written HIP kernels (salsa_amd/csrc/attention.hip, C ABI in include/salsa_nn.h): the attention core
directly on the in-projection's packed (B, T, 3, heads, dh) output, and the fused residual add + LayerNorm.  All float32."""
import ctypes as C
import os

import torch
import torch.nn.functional as F

from .. import _lib
from .fused_gru import _stream

HIP_ATTN = os.environ.get('SALSA_HIP_ATTN', '1') != '0'   # 0: nn.MultiheadAttention / F.layer_norm in the blocks, for A/B runs and bisecting


def attn_supported(T, n_heads, head_dim):
    return bool(_lib.load().salsa_nn_attn_supported(int(T), int(n_heads), int(head_dim)))


class _AttnCore(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, n_heads):
        """qkv (B, T, 3 * n_heads * dh) float32 -> out (B, T, n_heads * dh)"""
        qkv = qkv.contiguous()
        B, T, E3 = qkv.shape
        dh = E3 // (3 * n_heads)
        out = torch.empty((B, T, n_heads * dh), dtype=torch.float32, device=qkv.device)
        lse = torch.empty((B, n_heads, T), dtype=torch.float32, device=qkv.device)
        with torch.cuda.device(qkv.device):
            rc = _lib.load().salsa_nn_attn_fwd(C.c_void_p(qkv.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(lse.data_ptr()),
                                               B, T, n_heads, dh, _stream(qkv))
        if rc:
            raise RuntimeError('salsa_nn_attn_fwd failed (%d) for B %d, T %d, %d heads of %d' % (rc, B, T, n_heads, dh))
        ctx.n_heads = n_heads
        ctx.save_for_backward(qkv, out, lse)
        return out

    @staticmethod
    def backward(ctx, d_out):
        qkv, out, lse = ctx.saved_tensors
        B, T, E3 = qkv.shape
        dh = E3 // (3 * ctx.n_heads)
        d_out = d_out.contiguous()
        d_qkv = torch.empty_like(qkv)
        with torch.cuda.device(qkv.device):
            rc = _lib.load().salsa_nn_attn_bwd(C.c_void_p(qkv.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(lse.data_ptr()),
                                               C.c_void_p(d_out.data_ptr()), C.c_void_p(d_qkv.data_ptr()), B, T, ctx.n_heads, dh,
                                               _stream(qkv))
        if rc:
            raise RuntimeError('salsa_nn_attn_bwd failed (%d)' % rc)
        return d_qkv, None


def attn_core(qkv, n_heads):
    """softmax(q k^T / sqrt(dh)) v per head on the packed in-projection output: qkv (B, T, 3 * n_heads * dh) float32 CUDA, read as
    (B, T, 3, n_heads, dh) -> (B, T, n_heads * dh), ready for the out-projection.  Differentiable (salsa_nn_attn_fwd / _bwd)."""
    if not (qkv.is_cuda and qkv.dtype == torch.float32 and qkv.dim() == 3 and qkv.shape[2] % (3 * n_heads) == 0):
        raise ValueError('attn_core: float32 CUDA (B, T, 3 * n_heads * dh) expected, got %s %s' % (qkv.dtype, tuple(qkv.shape)))
    return _AttnCore.apply(qkv, n_heads)


class _AddLayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, res, weight, bias, eps):
        x, res = x.contiguous(), res.contiguous()
        Cn = x.shape[-1]
        M = x.numel() // Cn
        y = torch.empty_like(x)
        stats = torch.empty((2, M), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            rc = _lib.load().salsa_nn_add_layernorm_fwd(C.c_void_p(x.data_ptr()), C.c_void_p(res.data_ptr()),
                                                        C.c_void_p(weight.contiguous().data_ptr()), C.c_void_p(bias.contiguous().data_ptr()),
                                                        C.c_void_p(y.data_ptr()), C.c_void_p(stats[0].data_ptr()),
                                                        C.c_void_p(stats[1].data_ptr()), M, Cn, float(eps), _stream(x))
        if rc:
            raise RuntimeError('salsa_nn_add_layernorm_fwd failed (%d) for M %d, C %d' % (rc, M, Cn))
        ctx.save_for_backward(x, res, weight, stats)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, res, weight, stats = ctx.saved_tensors
        Cn = x.shape[-1]
        M = x.numel() // Cn
        dy = dy.contiguous()
        L = _lib.load()
        dx = torch.empty_like(x)
        dwb = torch.empty((2, Cn), dtype=torch.float32, device=x.device)
        ws_bytes = L.salsa_nn_add_layernorm_ws_bytes(M, Cn)
        ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            rc = L.salsa_nn_add_layernorm_bwd(C.c_void_p(dy.data_ptr()), C.c_void_p(x.data_ptr()), C.c_void_p(res.data_ptr()),
                                              C.c_void_p(weight.contiguous().data_ptr()), C.c_void_p(stats[0].data_ptr()),
                                              C.c_void_p(stats[1].data_ptr()), C.c_void_p(dx.data_ptr()), C.c_void_p(dwb[0].data_ptr()),
                                              C.c_void_p(dwb[1].data_ptr()), C.c_void_p(ws.data_ptr()), ws_bytes, M, Cn, _stream(x))
        if rc:
            raise RuntimeError('salsa_nn_add_layernorm_bwd failed (%d)' % rc)
        return dx, dx, dwb[0], dwb[1], None


def add_layernorm_supported(x):
    return x.is_cuda and x.dtype == torch.float32 and x.shape[-1] in (256, 512) and x.numel() > 0


def add_layernorm(x, res, weight, bias, eps=1e-5):
    """LayerNorm(x + res) over the last axis (C = 256 or 512), float32 CUDA; differentiable in x, res, weight and bias
    (salsa_nn_add_layernorm_fwd / _bwd; the gradients of x and res are one tensor)."""
    if not (add_layernorm_supported(x) and res.shape == x.shape and res.dtype == x.dtype and res.device == x.device):
        raise ValueError('add_layernorm: float32 CUDA (..., 256 | 512) pairs expected, got %s and %s' % (tuple(x.shape), tuple(res.shape)))
    return _AddLayerNorm.apply(x, res, weight, bias, eps)


def attn_block_forward(block, x, training):
    """One AttnBlock on x (B, T, d) float32: norm(x + drop(mha(x, x, x)[0])).  On the GPU with SALSA_HIP_ATTN=1 and a supported shape:
    in-projection GEMM -> attn_core -> out-projection GEMM -> dropout (torch's) -> add_layernorm; otherwise the torch modules."""
    mha, norm = block.mha, block.norm
    if not (HIP_ATTN and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and add_layernorm_supported(x)
            and attn_supported(x.shape[1], mha.num_heads, mha.head_dim)):
        return norm(x + block.drop(mha(x, x, x, need_weights=False)[0]))
    qkv = F.linear(x, mha.in_proj_weight, mha.in_proj_bias)                 # (B, T, 3 d) = (B, T, 3, heads, dh)
    a = F.linear(attn_core(qkv, mha.num_heads), mha.out_proj.weight, mha.out_proj.bias)
    if training and block.drop.p > 0:
        a = torch.dropout(a, block.drop.p, True)
    return add_layernorm(a, x, norm.weight, norm.bias, norm.eps)
