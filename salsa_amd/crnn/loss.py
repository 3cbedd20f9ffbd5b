"""SELD training losses.  reg_xyz (models/interfaces.py:304-355): 0.3 * BCE-with-logits(SED) + 0.7 * sum over x,y,z of the
activity-masked mean absolute error.  accdoa (:273-302): the activity-masked squared error of the xyz output over all rows.
multi_accdoa (no reference code): auxiliary duplicating permutation-invariant training over three tracks per
class."""
import os

import torch
import torch.nn.functional as F

FUSED_LOSS = os.environ.get('SALSA_FUSED_LOSS', '1') == '1'   # one HIP launch for the loss and its gradients (CUDA tensors)


def masked_mae(pred, target, mask):
    n = min(pred.shape[1], target.shape[1])
    pred, target, mask = pred[:, :n], target[:, :n], mask[:, :n]
    return torch.sum(torch.abs(pred - target) * mask) / torch.sum(mask)


def seld_loss(pred, sed_gt, doa_gt, loss_weight=(0.3, 0.7)):
    """pred: dict from SeldCRNN; sed_gt (B,T,12); doa_gt (B,T,36) -> (loss, sed_loss, doa_loss)."""
    nc = sed_gt.shape[-1]
    logit, doa = pred['event_frame_logit'].float(), pred['doa_frame_output'].float()
    if (FUSED_LOSS and logit.is_cuda and sed_gt.dtype == torch.float32 and doa_gt.dtype == torch.float32
            and logit.shape == sed_gt.shape and doa.shape == doa_gt.shape and doa.shape[-1] == 3 * nc):
        out = _SeldLoss.apply(logit, doa, sed_gt, doa_gt, float(loss_weight[0]), float(loss_weight[1]))
        return out[0], out[1], out[2]
    sed = F.binary_cross_entropy_with_logits(logit, sed_gt)
    d = sum(masked_mae(doa[..., i * nc:(i + 1) * nc], doa_gt[..., i * nc:(i + 1) * nc], sed_gt) for i in range(3))
    return loss_weight[0] * sed + loss_weight[1] * d, sed, d


class _SeldLoss(torch.autograd.Function):
    """salsa_nn_seld_loss: the loss above and its gradients in ONE launch (the eager version is ~35 kernels of a few
    microseconds on 30 k-element tensors), one more launch in the backward to scale them by the incoming gradients."""

    @staticmethod
    def forward(ctx, logit, doa, sed_gt, doa_gt, w_sed, w_doa):
        from .. import _lib
        from .nn_ops import _ptr, _stream
        logit, doa, sed_gt, doa_gt = logit.contiguous(), doa.contiguous(), sed_gt.contiguous(), doa_gt.contiguous()
        nc = sed_gt.shape[-1]
        rows = sed_gt.numel() // nc
        out = torch.empty(3, dtype=torch.float32, device=logit.device)
        ws = torch.empty(192, dtype=torch.float64, device=logit.device)       # include/salsa_nn.h SALSA_SELD_LOSS_WS
        ga, gb = torch.empty_like(logit), torch.empty_like(doa)
        with torch.cuda.device(logit.device):
            rc = _lib.load().salsa_nn_seld_loss(_ptr(logit), _ptr(doa), _ptr(sed_gt), _ptr(doa_gt), rows, nc, w_sed, w_doa, _ptr(out),
                                                _ptr(ga), _ptr(gb), _ptr(ws), _stream(logit))
        if rc:
            raise RuntimeError('salsa_nn_seld_loss failed (%d)' % rc)
        ctx.set_materialize_grads(False)          # unused outputs (the two detached parts) arrive as None, not as zero fills
        ctx.save_for_backward(ga, gb)
        ctx.w = (w_sed, w_doa)
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, g_loss, g_sed, g_doa):
        from .. import _lib
        from .nn_ops import _ptr, _stream
        ga, gb = ctx.saved_tensors
        if g_loss is None and g_sed is None and g_doa is None:
            return None, None, None, None, None, None
        oa, ob = torch.empty_like(ga), torch.empty_like(gb)

        def scalar(g):
            return None if g is None else g.to(device=ga.device, dtype=torch.float32).contiguous()
        g_loss, g_sed, g_doa = scalar(g_loss), scalar(g_sed), scalar(g_doa)
        with torch.cuda.device(ga.device):
            rc = _lib.load().salsa_nn_seld_loss_bwd(_ptr(ga), ga.numel(), _ptr(gb), gb.numel(), _ptr(g_loss), _ptr(g_sed), _ptr(g_doa),
                                                    ctx.w[0], ctx.w[1], _ptr(oa), _ptr(ob), _stream(ga))
        if rc:
            raise RuntimeError('salsa_nn_seld_loss_bwd failed (%d)' % rc)
        return oa, ob, None, None, None, None


def accdoa_loss(pred, sed_gt, doa_gt):
    """output_format 'accdoa' (compute_loss :273-282, compute_classwise_accdoa_loss :284-302): pred: dict from SeldCRNN; sed_gt
    (B,T,C); doa_gt (B,T,3C) -> (loss, sed_loss, doa_loss) with doa_loss = sum(((p - t)^2 summed over x, y, z) * sed_gt) / (B T),
    loss = doa_loss and sed_loss = 0 (the reference computes a sed term and discards it; loss_weight is not used).  The event
    logits are not part of the loss, but they get an exact-zero gradient: with every parameter holding a gradient the bucketed
    all-reduce and DDP see the same parameters as under reg_xyz, and Adam (weight_decay 0) leaves the event head unchanged, as
    the reference's grad = None does."""
    nc = sed_gt.shape[-1]
    logit, doa = pred.get('event_frame_logit'), pred['doa_frame_output'].float()
    if (FUSED_LOSS and doa.is_cuda and sed_gt.dtype == torch.float32 and doa_gt.dtype == torch.float32 and logit is not None
            and logit.shape == sed_gt.shape and doa.shape == doa_gt.shape and doa.shape[-1] == 3 * nc):
        out = _AccdoaLoss.apply(logit.float(), doa, sed_gt, doa_gt)
        return out[0], out[1], out[2]
    n = sed_gt.shape[0] * sed_gt.shape[1]
    e = (doa - doa_gt) ** 2
    d = torch.sum((e[..., :nc] + e[..., nc:2 * nc] + e[..., 2 * nc:]) * sed_gt) / n
    if logit is not None and logit.requires_grad:
        d = _ZeroGradTo.apply(d, logit)
    return d, torch.zeros((), dtype=d.dtype, device=d.device), d


class _ZeroGradTo(torch.autograd.Function):
    """y = x, and an exact-zero gradient for `other` (value untouched, whatever `other` holds: no 0 * other arithmetic)"""

    @staticmethod
    def forward(ctx, x, other):
        ctx.other = (other.shape, other.dtype, other.device)
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        shape, dtype, device = ctx.other
        return g, torch.zeros(shape, dtype=dtype, device=device)


class _AccdoaLoss(torch.autograd.Function):
    """salsa_nn_accdoa_loss: the accdoa loss, its gradient and the event logits' zero gradient in one call; the backward is
    salsa_nn_seld_loss_bwd with the weights (0, 1): g_logit stays zero, g_doa is scaled by g_loss + g_doa_loss."""

    @staticmethod
    def forward(ctx, logit, doa, sed_gt, doa_gt):
        from .. import _lib
        from .nn_ops import _ptr, _stream
        doa, sed_gt, doa_gt = doa.contiguous(), sed_gt.contiguous(), doa_gt.contiguous()
        nc = sed_gt.shape[-1]
        rows = sed_gt.numel() // nc
        out = torch.empty(3, dtype=torch.float32, device=doa.device)
        ws = torch.empty(64, dtype=torch.float64, device=doa.device)         # include/salsa_nn.h SALSA_ACCDOA_LOSS_WS
        ga, gb = torch.empty(logit.shape, dtype=torch.float32, device=doa.device), torch.empty_like(doa)
        with torch.cuda.device(doa.device):
            rc = _lib.load().salsa_nn_accdoa_loss(_ptr(doa), _ptr(sed_gt), _ptr(doa_gt), rows, nc, _ptr(out), _ptr(ga), _ptr(gb),
                                                  _ptr(ws), _stream(doa))
        if rc:
            raise RuntimeError('salsa_nn_accdoa_loss failed (%d)' % rc)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(ga, gb)
        ctx.w = (0.0, 1.0)
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, g_loss, g_sed, g_doa):
        return _SeldLoss.backward(ctx, g_loss, g_sed, g_doa)[:4]


# ADPIT's candidate assignments (track 0, 1, 2 -> source) by the number k of active slots, in index order; -1 is the zero target.
# k = 0 and k = 1 have one candidate, repeated here to a common length of six: an equal cost never displaces the first.
_ADPIT_CANDIDATES = (
    ((-1, -1, -1),) * 6,
    ((0, 0, 0),) * 6,
    ((0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0)),
    ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)),
)


def adpit_choose(doa, sed_gt, doa_gt):
    """The per-item rule of salsa_nn_adpit_loss in float64 torch operators: doa, doa_gt (..., 9 C), sed_gt (..., 3 C) -> (cost
    (rows, C, 6) float64 of the six candidates, chosen (rows, C) int64, d (rows, C, 6, 3, 3) = P - T per candidate, track, axis)."""
    C = sed_gt.shape[-1] // 3
    P = doa.double().reshape(-1, 3, 3, C).permute(0, 3, 2, 1)                  # (rows, C, track, axis)
    T = doa_gt.double().reshape(-1, 3, 3, C).permute(0, 3, 2, 1)               # (rows, C, slot, axis)
    s = sed_gt.reshape(-1, 3, C).permute(0, 2, 1) > 0.5                        # (rows, C, slot)
    order = torch.argsort((~s).to(torch.int8), dim=-1, stable=True)            # the active slots first, in slot order
    S = torch.gather(T, 2, order[..., None].expand(-1, -1, -1, 3))             # the sources (behind the k-th: not read)
    table = torch.tensor(_ADPIT_CANDIDATES, dtype=torch.long, device=doa.device)
    idx = table[s.sum(-1)]                                                     # (rows, C, 6, 3)
    tgt = torch.gather(S[:, :, None].expand(-1, -1, 6, -1, -1), 3, idx.clamp(min=0)[..., None].expand(-1, -1, -1, -1, 3))
    tgt = torch.where((idx < 0)[..., None], torch.zeros((), dtype=torch.float64, device=doa.device), tgt)
    d = P[:, :, None] - tgt
    cost = torch.zeros(d.shape[:3], dtype=torch.float64, device=doa.device)
    for n in range(3):                                                         # tracks outer, axes inner, one running sum
        for a in range(3):
            cost = cost + d[..., n, a] * d[..., n, a]
    best, chosen = cost[..., 0], torch.zeros(cost.shape[:2], dtype=torch.long, device=doa.device)
    for c in range(1, 6):                                                      # strictly smaller only: NaN never displaces
        better = cost[..., c] < best
        best, chosen = torch.where(better, cost[..., c], best), torch.where(better, torch.full_like(chosen, c), chosen)
    return cost, chosen, d


def adpit_loss(pred, sed_gt, doa_gt):
    """output_format 'multi_accdoa' (DESIGN.md section 9i): pred: dict from SeldCRNN(n_classes=3 C); sed_gt (B,T,3C) slot activities;
    doa_gt (B,T,9C) slot targets -> (loss, 0, loss): per (row, class) the least squared error over the ADPIT track assignments,
    / 9, averaged over rows x C (include/salsa_nn.h, salsa_nn_adpit_loss).  CUDA float32 tensors take the fused HIP launch; CPU
    tensors, and everything under SALSA_FUSED_LOSS=0, the same rule in float64 torch operators.  The event logits get an exact-zero
    gradient, as under accdoa."""
    nc3 = sed_gt.shape[-1]
    if nc3 % 3 != 0:
        raise ValueError('multi_accdoa labels hold three slots per class: %d columns' % nc3)
    logit, doa = pred.get('event_frame_logit'), pred['doa_frame_output'].float()
    if doa.shape[-1] != 3 * nc3 or doa.shape != doa_gt.shape:
        raise ValueError('multi_accdoa: prediction %s, sed_gt %s, doa_gt %s' % (tuple(doa.shape), tuple(sed_gt.shape), tuple(doa_gt.shape)))
    if (FUSED_LOSS and doa.is_cuda and sed_gt.dtype == torch.float32 and doa_gt.dtype == torch.float32 and logit is not None
            and logit.shape == sed_gt.shape and nc3 // 3 <= 1024):
        out = _AdpitLoss.apply(logit.float(), doa, sed_gt, doa_gt)
        return out[0], out[1], out[2]
    cost, chosen, _ = adpit_choose(doa, sed_gt, doa_gt)
    e_min = torch.gather(cost, 2, chosen[..., None])[..., 0]
    d = ((e_min / 9.0).sum() / float(e_min.numel())).float()
    if logit is not None and logit.requires_grad:
        d = _ZeroGradTo.apply(d, logit)
    return d, torch.zeros((), dtype=d.dtype, device=d.device), d


class _AdpitLoss(torch.autograd.Function):
    """salsa_nn_adpit_loss: the ADPIT loss, its gradient and the event logits' zero gradient in one call; the backward is
    salsa_nn_seld_loss_bwd with the weights (0, 1), as for _AccdoaLoss."""

    @staticmethod
    def forward(ctx, logit, doa, sed_gt, doa_gt):
        from .. import _lib
        from .nn_ops import _ptr, _stream
        doa, sed_gt, doa_gt = doa.contiguous(), sed_gt.contiguous(), doa_gt.contiguous()
        nc3 = sed_gt.shape[-1]
        rows = sed_gt.numel() // nc3
        out = torch.empty(3, dtype=torch.float32, device=doa.device)
        ws = torch.empty(64, dtype=torch.float64, device=doa.device)         # include/salsa_nn.h SALSA_ADPIT_LOSS_WS
        ga, gb = torch.empty(logit.shape, dtype=torch.float32, device=doa.device), torch.empty_like(doa)
        with torch.cuda.device(doa.device):
            rc = _lib.load().salsa_nn_adpit_loss(_ptr(doa), _ptr(sed_gt), _ptr(doa_gt), rows, nc3 // 3, _ptr(out), _ptr(ga), _ptr(gb),
                                                 None, _ptr(ws), _stream(doa))
        if rc:
            raise RuntimeError('salsa_nn_adpit_loss failed (%d)' % rc)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(ga, gb)
        ctx.w = (0.0, 1.0)
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, g_loss, g_sed, g_doa):
        return _SeldLoss.backward(ctx, g_loss, g_sed, g_doa)[:4]
