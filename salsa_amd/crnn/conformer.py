"""The decoder's optional Conformer blocks: macaron feed-forward, self-attention, convolution module, second
feed-forward, each behind a pre-norm residual, and a closing LayerNorm.  The parameters live in plain torch modules (ConformerBlock
in model.py), so their initialisation, state-dict keys and the CPU path are torch's own.  On the GPU the eight projections stay GEMMs,
the attention step is attention.attn_core, and the rest runs on three hand-written HIP kernel families (salsa_amd/csrc/conformer.hip,
C ABI in include/salsa_nn.h): the residual + LayerNorm step with branch dropout, the bias + Swish + dropout epilogue of a feed-forward,
and the GLU -> depthwise convolution -> LayerNorm -> Swish core of the convolution module.  All float32.

Dropout masks are counter hashes of (element index, seed) regenerated in the backward; the seeds come from torch's CPU generator
(draw_seed), one per dropout site, drawn in this order in every block forward: FF1 inner, FF1 residual, attention residual,
convolution residual, FF2 inner, FF2 residual."""
import ctypes as C
import os

import torch
import torch.nn.functional as F

from .. import _lib
from .attention import attn_core, attn_supported
from .fused_gru import _stream

HIP_CONFORMER = os.environ.get('SALSA_HIP_CONFORMER', '1') != '0'   # 0: every step of a block on the torch modules, for A/B runs and bisecting


def draw_seed(p):
    """the mask seed of one dropout site from torch's CPU generator (torch.manual_seed makes it reproducible; no device sync)"""
    return int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) if p > 0 else 0


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _f32(x):
    return x.is_cuda and x.dtype == torch.float32 and x.numel() > 0


def res_layernorm_supported(x):
    return _f32(x) and bool(_lib.load().salsa_nn_res_layernorm_supported(x.numel() // x.shape[-1], x.shape[-1]))


def bias_swish_dropout_supported(a):
    return _f32(a) and bool(_lib.load().salsa_nn_bias_swish_dropout_supported(a.numel() // a.shape[-1], a.shape[-1]))


def conv_module_supported(a, kernel):
    return _f32(a) and a.dim() == 3 and a.shape[0] <= 65535 and bool(_lib.load().salsa_nn_conv_module_supported(a.shape[1], a.shape[2] // 2, kernel))


class _ResLayerNorm(torch.autograd.Function):
    """(z, y) = (x + scale * drop(branch), LayerNorm(z)); z is returned only when asked for.  Both gradients arrive in one backward."""

    @staticmethod
    def forward(ctx, x, branch, weight, bias, scale, p, seed, eps, want_z):
        x = x.contiguous()
        branch = branch.contiguous() if branch is not None else None
        weight, bias = weight.contiguous(), bias.contiguous()
        Cn = x.shape[-1]
        M = x.numel() // Cn
        y = torch.empty_like(x)
        z = torch.empty_like(x) if want_z else None
        stats = torch.empty((2, M), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            rc = _lib.load().salsa_nn_res_layernorm_fwd(_ptr(x), _ptr(branch), float(scale), float(p), seed, _ptr(weight), _ptr(bias), _ptr(z),
                                                        _ptr(y), _ptr(stats[0]), _ptr(stats[1]), M, Cn, float(eps), _stream(x))
        if rc:
            raise RuntimeError('salsa_nn_res_layernorm_fwd failed (%d) for M %d, C %d' % (rc, M, Cn))
        ctx.save_for_backward(x, branch, weight, stats)
        ctx.args = (float(scale), float(p), seed)
        ctx.set_materialize_grads(False)
        return (z, y) if want_z else y

    @staticmethod
    def backward(ctx, *grads):
        dz, dy = grads if len(grads) == 2 else (None, grads[0])
        x, branch, weight, stats = ctx.saved_tensors
        if dz is None and dy is None:
            return (None,) * 9
        scale, p, seed = ctx.args
        Cn = x.shape[-1]
        M = x.numel() // Cn
        dz = dz.contiguous() if dz is not None else None
        dy = dy.contiguous() if dy is not None else None
        L = _lib.load()
        dx = torch.empty_like(x)
        # the branch's gradient is dx itself when nothing scales or masks it: one tensor serves both
        own = branch is not None and (scale != 1.0 or p > 0)
        dbranch = torch.empty_like(x) if own else None
        dwb = torch.empty((2, Cn), dtype=torch.float32, device=x.device) if dy is not None else None
        ws_bytes = L.salsa_nn_res_layernorm_ws_bytes(M, Cn)
        ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=x.device) if dy is not None else None
        with torch.cuda.device(x.device):
            rc = L.salsa_nn_res_layernorm_bwd(_ptr(dy), _ptr(dz), _ptr(x), _ptr(branch), scale, p, seed, _ptr(weight), _ptr(stats[0]),
                                              _ptr(stats[1]), _ptr(dx), _ptr(dbranch), _ptr(dwb[0]) if dy is not None else None,
                                              _ptr(dwb[1]) if dy is not None else None, _ptr(ws), ws_bytes, M, Cn, _stream(x))
        if rc:
            raise RuntimeError('salsa_nn_res_layernorm_bwd failed (%d)' % rc)
        gb = None if branch is None else dbranch if own else dx
        return dx, gb, (dwb[0] if dy is not None else None), (dwb[1] if dy is not None else None), None, None, None, None, None


def res_layernorm(x, branch, norm, scale=1.0, p=0.0, want_z=True):
    """z = x + scale * dropout(branch, p) (branch None: z = x) and y = norm(z) over the last axis -> (z, y), or y alone with
    want_z=False.  norm: an nn.LayerNorm.  The HIP step (salsa_nn_res_layernorm_fwd / _bwd) on float32 CUDA rows of 256 or 512 with
    SALSA_HIP_CONFORMER=1, torch's operators otherwise (p = 0 outside training is the caller's business)."""
    if HIP_CONFORMER and res_layernorm_supported(x):
        seed = draw_seed(p if branch is not None else 0.0)
        return _ResLayerNorm.apply(x, branch, norm.weight, norm.bias, scale, p, seed, norm.eps, want_z)
    z = x if branch is None else x + scale * F.dropout(branch, p, p > 0)
    y = F.layer_norm(z, (z.shape[-1],), norm.weight, norm.bias, norm.eps)
    return (z, y) if want_z else y


class _BiasSwishDropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, bias, p, seed):
        a, bias = a.contiguous(), bias.contiguous()
        Cn = a.shape[-1]
        M = a.numel() // Cn
        h = torch.empty_like(a)
        with torch.cuda.device(a.device):
            rc = _lib.load().salsa_nn_bias_swish_dropout_fwd(_ptr(a), _ptr(bias), _ptr(h), M, Cn, float(p), seed, _stream(a))
        if rc:
            raise RuntimeError('salsa_nn_bias_swish_dropout_fwd failed (%d) for M %d, C %d' % (rc, M, Cn))
        ctx.save_for_backward(a, bias)
        ctx.args = (float(p), seed)
        return h

    @staticmethod
    def backward(ctx, dh):
        a, bias = ctx.saved_tensors
        p, seed = ctx.args
        Cn = a.shape[-1]
        M = a.numel() // Cn
        dh = dh.contiguous()
        L = _lib.load()
        da, db = torch.empty_like(a), torch.empty_like(bias)
        ws_bytes = L.salsa_nn_bias_swish_dropout_ws_bytes(M, Cn)
        ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=a.device)
        with torch.cuda.device(a.device):
            rc = L.salsa_nn_bias_swish_dropout_bwd(_ptr(dh), _ptr(a), _ptr(bias), _ptr(da), _ptr(db), _ptr(ws), ws_bytes, M, Cn, p, seed,
                                                   _stream(a))
        if rc:
            raise RuntimeError('salsa_nn_bias_swish_dropout_bwd failed (%d)' % rc)
        return da, db, None, None


def bias_swish_dropout(a, bias, p=0.0):
    """dropout(swish(a + bias), p) on (..., C): the epilogue of a feed-forward's first GEMM, which runs WITHOUT its bias -- it enters
    here, and its gradient is the kernel's fixed-order column sum (salsa_nn_bias_swish_dropout_fwd / _bwd)."""
    if HIP_CONFORMER and bias_swish_dropout_supported(a):
        return _BiasSwishDropout.apply(a, bias, p, draw_seed(p))
    return F.dropout(F.silu(a + bias), p, p > 0)


class _ConvModule(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, dw_weight, dw_bias, weight, bias, eps):
        a, dw_weight, dw_bias, weight, bias = (t.contiguous() for t in (a, dw_weight, dw_bias, weight, bias))
        B, T, d2 = a.shape
        d, kernel = d2 // 2, dw_weight.shape[-1]
        u = torch.empty((B, T, d), dtype=torch.float32, device=a.device)
        with torch.cuda.device(a.device):
            rc = _lib.load().salsa_nn_conv_module_fwd(_ptr(a), _ptr(dw_weight), _ptr(dw_bias), _ptr(weight), _ptr(bias), _ptr(u), B, T, d, kernel,
                                                      float(eps), _stream(a))
        if rc:
            raise RuntimeError('salsa_nn_conv_module_fwd failed (%d) for B %d, T %d, d %d, kernel %d' % (rc, B, T, d, kernel))
        ctx.save_for_backward(a, dw_weight, dw_bias, weight, bias)
        ctx.eps = float(eps)
        return u

    @staticmethod
    def backward(ctx, du):
        a, dw_weight, dw_bias, weight, bias = ctx.saved_tensors
        B, T, d2 = a.shape
        d, kernel = d2 // 2, dw_weight.shape[-1]
        du = du.contiguous()
        L = _lib.load()
        da, dw = torch.empty_like(a), torch.empty_like(dw_weight)
        small = torch.empty((3, d), dtype=torch.float32, device=a.device)
        ws_bytes = L.salsa_nn_conv_module_ws_bytes(B, T, d, kernel)
        ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=a.device)
        with torch.cuda.device(a.device):
            rc = L.salsa_nn_conv_module_bwd(_ptr(du), _ptr(a), _ptr(dw_weight), _ptr(dw_bias), _ptr(weight), _ptr(bias), _ptr(da), _ptr(dw),
                                            _ptr(small[0]), _ptr(small[1]), _ptr(small[2]), _ptr(ws), ws_bytes, B, T, d, kernel, ctx.eps,
                                            _stream(a))
        if rc:
            raise RuntimeError('salsa_nn_conv_module_bwd failed (%d)' % rc)
        return da, dw, small[0], small[1], small[2], None


def conv_module_core(a, dw, norm):
    """swish(norm(dw(glu(a)))) along time: a (B, T, 2 d) -> (B, T, d); dw: the depthwise nn.Conv1d, norm: its nn.LayerNorm
    (salsa_nn_conv_module_fwd / _bwd for d 256 / 512 and T <= 512 with SALSA_HIP_CONFORMER=1, torch's operators otherwise)."""
    if HIP_CONFORMER and conv_module_supported(a, dw.kernel_size[0]):
        return _ConvModule.apply(a, dw.weight, dw.bias, norm.weight, norm.bias, norm.eps)
    v = dw(F.glu(a, dim=-1).transpose(1, 2)).transpose(1, 2)
    return F.silu(F.layer_norm(v, (v.shape[-1],), norm.weight, norm.bias, norm.eps))


def _feed_forward(n, w1, w2, p):
    return F.linear(bias_swish_dropout(F.linear(n, w1.weight), w1.bias, p), w2.weight, w2.bias)


def _self_attention(mha, n):
    if attn_supported(n.shape[1], mha.num_heads, mha.head_dim):
        qkv = F.linear(n, mha.in_proj_weight, mha.in_proj_bias)             # (B, T, 3 d) = (B, T, 3, heads, dh)
        return F.linear(attn_core(qkv, mha.num_heads), mha.out_proj.weight, mha.out_proj.bias)
    return mha(n, n, n, need_weights=False)[0]


def block_forward(block, x, training):
    """One ConformerBlock on x (B, T, d) float32.  On the GPU with SALSA_HIP_CONFORMER=1: 5 residual / LayerNorm launches, 2 feed-forward
    epilogues, 1 attention core, 1 convolution module and 8 GEMMs; a step whose shape its kernel does not take falls back to the torch
    form of that step alone.  Otherwise the torch modules (ConformerBlock.forward_torch, the same definition)."""
    if not (HIP_CONFORMER and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3):
        return block.forward_torch(x)
    p = block.drop.p if training else 0.0
    n = res_layernorm(x, None, block.norm_ff1, want_z=False)
    x, n = res_layernorm(x, _feed_forward(n, block.ff1_w1, block.ff1_w2, p), block.norm_att, 0.5, p)
    x, n = res_layernorm(x, _self_attention(block.mha, n), block.norm_conv, 1.0, p)
    c = F.linear(conv_module_core(F.linear(n, block.conv_p1.weight, block.conv_p1.bias), block.conv_dw, block.conv_norm),
                 block.conv_p2.weight, block.conv_p2.bias)
    x, n = res_layernorm(x, c, block.norm_ff2, 1.0, p)
    return res_layernorm(x, _feed_forward(n, block.ff2_w1, block.ff2_w2, p), block.norm_out, 0.5, p, want_z=False)
