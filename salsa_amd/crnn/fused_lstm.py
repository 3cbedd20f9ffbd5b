"""The decoder's recurrent layers for every decoder_type but 'bigru' (which keeps fused_gru.bigru_forward): nn.GRU and nn.LSTM,
one or two directions, with the time recurrence as ONE hand-written HIP launch per layer (GRU: salsa_amd/csrc/gru_scan.hip,
LSTM: salsa_amd/csrc/lstm_scan.hip; C ABI in include/salsa_gru.h).  The input projection and the weight gradients stay GEMMs
as in fused_gru.  Parameters are read from the torch module, so state dicts are unchanged.

The LSTM has no register-resident scan (4H x H float16 at H = 256 fills a whole workgroup's register file): it runs the float32
streaming kernels in training and inference, under bf16 autocast as well."""
import ctypes as C
import os

import torch

from .. import _lib
from .fused_gru import LEAN, REGISTER_WEIGHTS, _bias_grad, _GruScan, _InputProjection, _scan_inference, _stream

FUSED_LSTM = os.environ.get('SALSA_FUSED_LSTM', '1') != '0'   # 0: nn.LSTM (MIOpen) in the decoder, for A/B runs and bisecting


class _LstmScan(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gi, whh, bhh):
        """gi (T,B,D,4H) float32 contiguous; whh (D,4H,H); bhh (D,4H) -> hs (T,B,D,H)."""
        T, B, D, H4 = gi.shape
        H = H4 // 4
        whh = whh.contiguous()
        hs = torch.empty((T, B, D, H), dtype=torch.float32, device=gi.device)
        need_grad = gi.requires_grad or whh.requires_grad or bhh.requires_grad
        saved = torch.empty((T, B, D, 5 * H), dtype=torch.float32, device=gi.device) if need_grad else None
        whh_t = whh.transpose(1, 2).contiguous()
        with torch.cuda.device(gi.device):
            rc = _lib.load().salsa_lstm_scan_fwd(C.c_void_p(gi.data_ptr()), C.c_void_p(whh_t.data_ptr()),
                                                 C.c_void_p(bhh.contiguous().data_ptr()), C.c_void_p(hs.data_ptr()),
                                                 C.c_void_p(saved.data_ptr() if saved is not None else 0), T, B, D, H, _stream(gi))
        if rc:
            raise RuntimeError('salsa_lstm_scan_fwd failed (%d)' % rc)
        if need_grad:
            ctx.save_for_backward(whh, hs, saved)
        return hs

    @staticmethod
    def backward(ctx, dhs):
        whh, hs, saved = ctx.saved_tensors
        T, B, D, H = hs.shape
        dhs = dhs.contiguous()
        dg = torch.empty((T, B, D, 4 * H), dtype=torch.float32, device=hs.device)
        with torch.cuda.device(hs.device):
            rc = _lib.load().salsa_lstm_scan_bwd(C.c_void_p(dhs.data_ptr()), C.c_void_p(whh.data_ptr()), C.c_void_p(saved.data_ptr()),
                                                 C.c_void_p(dg.data_ptr()), T, B, D, H, _stream(hs))
        if rc:
            raise RuntimeError('salsa_lstm_scan_bwd failed (%d)' % rc)
        # the gradient wrt W_hh h_prev + b_hh is dg itself; dW_hh as in _GruScan.backward: one GEMM per direction on shifted views
        # (h before step t is hs[t - 1] forward, hs[t + 1] in reverse, zero at the scan's first step)
        dwhh = torch.empty((D, 4 * H, H), dtype=torch.float32, device=hs.device)
        if T > 1:
            torch.mm(dg[1:, :, 0].reshape(-1, 4 * H).t(), hs[:-1, :, 0].reshape(-1, H), out=dwhh[0])
            if D > 1:
                torch.mm(dg[:-1, :, 1].reshape(-1, 4 * H).t(), hs[1:, :, 1].reshape(-1, H), out=dwhh[1])
        else:
            dwhh.zero_()
        dbhh = _bias_grad(dg.view(T * B, D * 4 * H), (D, 4 * H))
        return dg, dwhh, dbhh


def rnn_forward(rnn: torch.nn.RNNBase, x: torch.Tensor, training: bool, half_weights: bool = False) -> torch.Tensor:
    """x (B,T,In) float32 CUDA -> (B,T,D*H); equivalent to ``rnn(x)[0]`` for a batch_first nn.GRU or nn.LSTM with biases, one or
    two directions, any number of layers (inter-layer dropout as torch places it: on every layer's input but the first, in
    training).  half_weights (the caller is under bf16 autocast): a GRU with H = 256 runs the register-resident scans (W_hh as
    float16), as bigru_forward does; the LSTM always runs the float32 streaming scans."""
    assert rnn.batch_first and rnn.bias and isinstance(rnn, (torch.nn.GRU, torch.nn.LSTM)) and rnn.proj_size == 0
    from .nn_ops import stack_groups
    is_lstm = isinstance(rnn, torch.nn.LSTM)
    names = ('', '_reverse') if rnn.bidirectional else ('',)
    out = x.transpose(0, 1).contiguous()        # time-major between the layers: the scans' order
    for layer in range(rnn.num_layers):
        wih, whh, bih, bhh = stack_groups([[getattr(rnn, '%s_l%d%s' % (kind, layer, n)) for n in names]   # (D,G,In), (D,G,H), (D,G) x 2
                                           for kind in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')])
        if layer > 0 and training and rnn.dropout > 0:
            out = torch.nn.functional.dropout(out, p=rnn.dropout, training=True)
        gi = _InputProjection.apply(out, wih, bih) if (out.is_cuda and LEAN) else \
            (torch.einsum('tbi,dgi->tbdg', out, wih) + bih).contiguous()           # (T,B,D,G)
        if is_lstm:
            hs = _LstmScan.apply(gi, whh, bhh)
        else:
            no_grad = not (torch.is_grad_enabled() and (gi.requires_grad or whh.requires_grad))
            regw = REGISTER_WEIGHTS and half_weights and whh.shape[2] == 256
            hs = _scan_inference(gi, whh, bhh) if (regw and no_grad) else _GruScan.apply(gi, whh, bhh, regw)
        out = hs.view(hs.shape[0], hs.shape[1], -1)                                 # (T, B, D*H)
    return out.transpose(0, 1)                                                      # (B, T, D*H), a view
