"""Float64 references for the CRNN kernels (conv_wide.hip, conv_mfma.hip, conv_1x1.hip, nn_pool.hip, nn_batchnorm.hip, gru_scan.hip) and the
per-element error bounds the tests hold them to.

Every reference takes the operands the kernel saw (bf16 values cast up exactly) and evaluates in float64 on their device,
so its own error is ~2^-53 relative and negligible.  A bound is never a multiple of max|ref|: it is built per element from
the magnitudes that enter that element's floating-point chain, so a kernel that drops one term where the terms are large,
or shifts every element by a small relative amount, still fails.

Unit roundoff u = 2^-24 (float32).  The standard result for a sum of n terms added one after another in float32 is
|computed - exact| <= (n - 1) u sum|term| (first order; Higham, Accuracy and Stability of Numerical Algorithms, 4.2), and a
tree of depth d gives d u sum|term|.  The constants below are those chain lengths, counted from the kernels' code.
"""
import math

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24            # float32 unit roundoff
BF16_REL = 2.0 ** -8        # bf16 unit roundoff: rounding to bf16 moves a value by at most 2^-8 of itself (8-bit significand)
_CHUNK_PIX = 1 << 15        # pixels per unfold chunk (memory stays ~ 32 Ki x 9 Cin doubles)


def _chunks(n, hw):
    step = max(1, _CHUNK_PIX // hw)
    return [(i, min(n, i + step)) for i in range(0, n, step)]


def conv_fwd_ref(x, w, shift=None, residual=None, relu=False):
    """(ref, absum) float64 (N, Cout, H, W): ref = [relu](conv(x, w) + shift + residual) with 'same' padding (k = 1 or 3),
    absum = sum |w x| over the products + |shift| + |residual| (the magnitudes in the element's float32 chain)."""
    k = w.shape[-1]
    N, _, H, W = x.shape
    wd = w.double().reshape(w.shape[0], -1)
    wa = wd.abs()
    ref = torch.empty((N, w.shape[0], H, W), dtype=torch.float64, device=x.device)
    absum = torch.empty_like(ref)
    for a, b in _chunks(N, H * W):
        xc = x[a:b].double()
        cols = F.unfold(xc, k, padding=k // 2) if k > 1 else xc.reshape(b - a, xc.shape[1], H * W)   # (n, Cin k k, HW)
        ref[a:b] = torch.matmul(wd, cols).view(b - a, -1, H, W)
        absum[a:b] = torch.matmul(wa, cols.abs()).view(b - a, -1, H, W)
    if shift is not None:
        ref += shift.double().view(1, -1, 1, 1)
        absum += shift.double().abs().view(1, -1, 1, 1)
    if residual is not None:
        ref += residual.double()
        absum += residual.double().abs()
    if relu:
        ref.clamp_(min=0)
    return ref, absum


_STREAM_PIX = 1 << 17       # pixels per piece of conv_fwd_ref_stream (its unfold: 128 Ki x 9 Cin doubles, twice)


def conv_fwd_ref_stream(x, w, shift=None, residual=None, relu=False, pool=False, max_pix=_STREAM_PIX):
    """conv_fwd_ref piece by piece, for maps whose whole-batch float64 tensors must never exist (32 x 64 x 4800 x 200: 2 x 15.7
    GB).  Yields ((n, h0, h1), ref, absum): clip n, OUTPUT rows h0 .. h1 - 1, ref / absum float64 (1, Cout, h1 - h0, Wout).  A
    piece is a band of at most max_pix input pixels of ONE clip; its one-row halo comes from the neighbouring rows of the same
    clip and is zero only at the clip's true top and bottom border, never the row of another clip or of a band's edge.
    pool=True (H and W even, bands of whole row pairs): ref = avgpool2x2([relu](conv + shift + residual)), absum = the 2x2 mean
    of the per-pixel absum; the bound of such an output is bf16_bound(ref, absum, pooled_conv_c(n_terms))."""
    k = w.shape[-1]
    p = k // 2
    N, _, H, W = x.shape
    assert not pool or (H % 2 == 0 and W % 2 == 0)
    wd = w.double().reshape(w.shape[0], -1)
    wa = wd.abs()
    step = max(1, max_pix // W)
    if pool:
        step = max(2, step - step % 2)
    sh = None if shift is None else shift.double().view(1, -1, 1, 1)
    for n in range(N):
        for h0 in range(0, H, step):
            h1 = min(H, h0 + step)
            lo, hi = max(0, h0 - p), min(H, h1 + p)
            xs = F.pad(x[n:n + 1, :, lo:hi].double(), (0, 0, lo - (h0 - p), (h1 + p) - hi))   # zero rows at the clip's border only
            cols = F.unfold(xs, k, padding=(0, p))                                            # (1, Cin k k, (h1 - h0) W)
            ref = torch.matmul(wd, cols).view(1, -1, h1 - h0, W)
            absum = torch.matmul(wa, cols.abs_()).view(1, -1, h1 - h0, W)
            del cols, xs
            if sh is not None:
                ref += sh
                absum += sh.abs()
            if residual is not None:
                r = residual[n:n + 1, :, h0:h1].double()
                ref += r
                absum += r.abs()
            if relu:
                ref.clamp_(min=0)
            if pool:
                yield (n, h0 // 2, h1 // 2), F.avg_pool2d(ref, 2), F.avg_pool2d(absum, 2)
            else:
                yield (n, h0, h1), ref, absum


def pooled_conv_c(n_terms):
    """c for salsa_nn_conv3x3_c64_bias_act_pool's output against conv_fwd_ref_stream(pool=True).  After the accumulator, the
    shift and the residual (conv_accum_c), conv64_epilogue<true> in conv_mfma.hip forms a pooled value from the four float32
    v = [relu](acc + shift + residual) as
        s = 0 + v(row 0); s += v(row 1)           one float32 addition (the first adds to 0: exact)
        s = 0.25 * (s + shfl_xor(s, 1))           one float32 addition; the product with 2^-2 is exact
    and rounds once to bf16: k = 2 additions, each within u of a partial sum of the four |v|, so 2 u sum|v| / 4 <= 2 u mean(absum)
    (|v| <= absum; ReLU is 1-Lipschitz and only shrinks |v|).  The four v's own accumulation errors, c absum each, average to
    c mean(absum).  Hence c = conv_accum_c(n_terms) + 2 u on the 2x2 mean of absum."""
    return conv_accum_c(n_terms) + 2 * U32


def avgpool_bound(x):
    """(ref, bound) of salsa_nn_avgpool2x2_fwd on bf16 input: avgpool2x2_fwd_kernel in nn_pool.hip forms (((a + b) + c) + d) / 4
    in float32 -- three additions, each within u of a partial sum <= sum|x|, an exact division by 4 -- and rounds once to
    bf16: |y - ref| <= 2^-8 |ref| + (1 + 2^-8) 3 u mean|x|."""
    xd = x.double()
    ref = F.avg_pool2d(xd, 2)
    return ref, BF16_REL * ref.abs() + (1 + BF16_REL) * 3 * U32 * F.avg_pool2d(xd.abs(), 2)


def avgpool_bwd_ref(gy, H, W):
    """float64 gradient of a floor-mode 2x2 average pool's (N, C, H, W) input for the pooled gradient gy: gy / 4 at the four
    pixels of a window, 0 in the last row of an odd H and the last column of an odd W.  avgpool2x2_bwd_kernel in nn_pool.hip
    forms g / 4.0f in float32 and rounds once: a division by 2^2 of a bf16 (or float32) value is exact in both formats (no
    rounding count; only a subnormal result could round), so the kernel's output EQUALS this reference cast to its dtype."""
    g = F.interpolate(gy.double(), scale_factor=2, mode='nearest') / 4
    return F.pad(g, (0, W - g.shape[3], 0, H - g.shape[2]))


def assert_dropped_plus_zero(g, what):
    """the (N, C, H, W) gradient of a floor-mode 2x2 pool's input holds +0.0 BIT FOR BIT in the last row of an odd H and the last
    column of an odd W: not -0.0, not the NaN the buffer was filled with (an element left unwritten), not a neighbour's value"""
    assert g.dtype in (torch.bfloat16, torch.float32)
    bits = g.view(torch.int16 if g.dtype == torch.bfloat16 else torch.int32)
    H, W = g.shape[2], g.shape[3]
    assert H % 2 or W % 2, what + ': the pool drops nothing at an even map'
    if W % 2:
        n = int((bits[:, :, :, W - 1] != 0).sum())
        assert n == 0, '%s: %d elements of the dropped last column are not +0.0' % (what, n)
    if H % 2:
        n = int((bits[:, :, H - 1, :] != 0).sum())
        assert n == 0, '%s: %d elements of the dropped last row are not +0.0' % (what, n)


def any_order_wgrad_bound(ref, absum, n_terms):
    """bound of a bf16 weight gradient whose float32 accumulation order is unknown (the torch / MIOpen fallback of a map the wide
    weight-gradient kernel refuses): ANY order of adding n_terms float32 products is within (n_terms - 1) u sum|term| of the
    exact sum (Higham 4.2 holds for every summation tree), then one rounding to bf16 as in bf16_bound."""
    return bf16_bound(ref, absum, (1 + BF16_REL) * (n_terms - 1) * U32)


def conv_wgrad_ref(x, gy, k=3):
    """(ref, absum) float64 (Cout, Cin, k, k): ref = sum over pixels of gy * x(shifted), absum = the same of |gy| |x|."""
    N, Cin, H, W = x.shape
    Cout = gy.shape[1]
    ref = torch.zeros((Cout, Cin * k * k), dtype=torch.float64, device=x.device)
    absum = torch.zeros_like(ref)
    for a, b in _chunks(N, H * W):
        xc = x[a:b].double()
        cols = F.unfold(xc, k, padding=k // 2) if k > 1 else xc.reshape(b - a, Cin, H * W)          # (n, Cin k k, HW)
        g = gy[a:b].double().reshape(b - a, Cout, H * W)
        ref += torch.einsum('npq,ncq->pc', g, cols)
        absum += torch.einsum('npq,ncq->pc', g.abs(), cols.abs())
    return ref.view(Cout, Cin, k, k), absum.view(Cout, Cin, k, k)


def flip_filter(w):
    """the data gradient's filter: w'[ci][co][r][s] = w[co][ci][2-r][2-s] (a Cout -> Cin convolution on dy)"""
    return w.flip(2, 3).transpose(0, 1)


def bf16_bound(ref, absum, c):
    """bound of a bf16 output whose float32 value v carries at most c * absum of accumulation error:
    |y - ref| <= |fl(v) - v| + |v - ref| <= 2^-8 |v| + c absum <= 2^-8 |ref| + (1 + 2^-8) c absum; c holds that spare factor."""
    return BF16_REL * ref.abs() + c * absum


def conv_accum_c(n_terms):
    """c for a float32 conv / GEMM output of n_terms products on the matrix cores: each MFMA step adds a 16-product dot
    product to the accumulator (products of bf16 are exact in float32; the 16-term sum counts as a 16-deep chain), so
    n_terms / 16 accumulator additions + 16, plus 2 for the epilogue's shift and residual adds."""
    return (math.ceil(n_terms / 16) + 16 + 2) * U32


def wide_wgrad_c(N, H, W, Cin, Cout):
    """c for salsa_nn_conv3x3_wide_wrw's float32 dW at one (N, H, W, Cin, Cout), from its summation chain:
    - the launch gives each of `shares` workgroups a contiguous run of ceil(tiles / shares) 128-pixel tiles, with
      shares = min(tiles, ceil(256 / ((Cout / 128) (Cin / 32)))), tiles = ceil(N H W / 128);
    - inside a workgroup the two wave groups (WG_KQ = 2) each take half of every tile's k-steps: an accumulator receives
      tiles_per_share * 128 / 2 / 16 MFMA updates of 16 products each (+16 for the in-MFMA sum);
    - the pair reduction adds the two halves (1);
    - the shares meet in dW by float32 atomics or, deterministic, by a sequential sum of the slabs (shares).
    Hence c = (tiles_per_share * 4 + 16 + 1 + shares) u.  At 32 x 160 x 50, 128 -> 128: shares 64, 32 tiles each, c = 209 u
    = 1.2e-5; a sequential float32 sum over all 256 000 pixels would need c = 256 000 u = 1.5e-2 -- a bound that loose
    would not see a missing 128-pixel tile (~sqrt(128) |gy x| against 1.5e-2 * 256 000 * E|gy x|)."""
    tiles = math.ceil(N * H * W / 128)
    pairs = (Cout // 128) * (Cin // 32)
    shares = max(1, min(tiles, math.ceil(256 / pairs)))
    per = math.ceil(tiles / shares)
    return (per * 128 // 2 // 16 + 16 + 1 + shares) * U32


def c64_wgrad_c(N, H, W):
    """c for salsa_nn_conv3x3_c64_wrw (64 -> 64): nb persistent workgroups (128 / 256 / 512 from 128 / 4096 / 16384 tiles of
    4 x 32 pixels up) each walk ceil(tiles / nb) tiles with an MFMA accumulator update per 16 pixels (8 per tile, + 16 for the
    in-MFMA sum), then the nb partials are added: c = (ceil(tiles / nb) * 8 + 16 + nb) u.  Tiles are counted per image on a
    grid rounded up to whole tiles."""
    tiles = N * math.ceil(H / 4) * math.ceil(W / 32)
    nb = 512 if tiles >= 16384 else 256 if tiles >= 4096 else 128 if tiles >= 128 else tiles
    return (math.ceil(tiles / nb) * 8 + 16 + nb) * U32


def conv1x1_wgrad_c(M, Cin, Cout):
    """c for salsa_nn_conv1x1_wrw: 64-pixel tiles, split = min(ceil(tiles / 2), max(1, 512 / ((Cout / 128) (Cin / 64))))
    workgroups along the pixels, each walking per = ceil(tiles / split) tiles with an MFMA step per 16 pixels, then the
    workgroups' partials are added (split): c = (per * 4 + 16 + split) u."""
    tiles = math.ceil(M / 64)
    split = max(1, 512 // ((Cout // 128) * (Cin // 64)))
    split = max(1, min(split, (tiles + 1) // 2))
    per = math.ceil(tiles / split)
    return (per * 4 + 16 + split) * U32


def check(got, ref, bound, what):
    """assert |got - ref| <= bound element-wise; returns max(|got - ref| / bound) for the report"""
    err = (got.double() - ref).abs()
    bad = ~(err <= bound)                                            # (a NaN fails)
    ratio = float((err / bound.clamp(min=1e-300)).max())
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError('%s: %d of %d elements outside the bound; first at %d: got %r ref %r bound %r (max err / bound %.3g)'
                             % (what, int(bad.sum()), bad.numel(), i, float(got.flatten()[i]), float(ref.flatten()[i]),
                                float(bound.flatten()[i]), ratio))
    return ratio


# ------------------------------------------------------------------------------------------------------------ BatchNorm
def bn_rows_per_thread(M, C, bf16):
    """upper bound of the float32 chain of one thread in nn_batchnorm.hip's reductions: a thread covers <= BN_RPT = 32 rows of a
    chunk, and with the grid capped at BN_MAX_BLOCKS = 1024 blocks of rpi = 256 / (C / L) rows it walks several chunks"""
    rpi = 256 // (C // (8 if bf16 else 4))
    return max(32, math.ceil(M / (rpi * 1024))) + int(math.log2(rpi)) + 2


def bn_train_ref(x, gamma, beta, eps, residual=None, relu=True, pool=False):
    """training-mode BatchNorm2d [+ residual] [+ ReLU] [-> 2x2 average pool] in float64.  Returns a dict: y, pre (the
    pre-activation), mean, var (biased), invstd, xhat, and fwd_abs: the magnitudes of y's float32 chain,
    |gamma| invstd (|x| + |mean|) + |beta| + |residual| + |gamma xhat| (1 + mean^2 / var)  -- the last term for the variance,
    whose float32 partial sums of squares carry BN_BATCH u (mean^2 + var) of error."""
    xd = x.double()
    M = xd.shape[0] * xd.shape[2] * xd.shape[3]
    mean = xd.mean(dim=(0, 2, 3))
    var = (xd * xd).mean(dim=(0, 2, 3)) - mean * mean
    invstd = 1.0 / torch.sqrt(var + eps)
    v = lambda t: t.view(1, -1, 1, 1)
    xhat = (xd - v(mean)) * v(invstd)
    g, b = gamma.double(), beta.double()
    pre = xhat * v(g) + v(b)
    fwd_abs = v(g.abs() * invstd) * (xd.abs() + v(mean.abs())) + v(b.abs()) + (xhat * v(g)).abs() * v(1 + mean * mean / var)
    if residual is not None:
        pre = pre + residual.double()
        fwd_abs = fwd_abs + residual.double().abs()
    y = pre.clamp(min=0) if relu else pre
    if pool:
        y = F.avg_pool2d(y, 2)
    return dict(y=y, pre=pre, mean=mean, var=var, unbiased=var * M / (M - 1), invstd=invstd, xhat=xhat, fwd_abs=fwd_abs, M=M)


def bn_eval_ref(x, gamma, beta, mean, invstd, residual=None, relu=True):
    """(ref, absum) float64 of salsa_nn_bn_eval_fwd: [relu]((x - mean) invstd gamma + beta [+ residual]) on the operands the
    kernel is handed (invstd is an operand: BatchNormAct2d.forward forms rsqrt(running_var + eps) in float32).  bn_apply_kernel in
    nn_batchnorm.hip evaluates ((x - mean) * invstd) * gamma + beta, + residual in float32: five roundings, each within u of a
    partial result <= absum = |gamma| invstd (|x| + |mean|) + |beta| + |residual|, so 5 u absum -- inside the 16 u the training
    forward (the same kernel, after its statistics) is held to; a bf16 output adds one rounding (bf16_bound)."""
    v = lambda t: t.double().view(1, -1, 1, 1)
    a = v(gamma) * v(invstd)
    ref = (x.double() - v(mean)) * a + v(beta)
    absum = a.abs() * (x.double().abs() + v(mean).abs()) + v(beta).abs()
    if residual is not None:
        ref = ref + residual.double()
        absum = absum + residual.double().abs()
    return (ref.clamp_(min=0) if relu else ref), absum


def bn_bwd_ref(r, gamma, gy, relu=True, pool=False, fwd_c=16 * U32, bf16=False):
    """float64 gradients of bn_train_ref's output for an upstream gradient gy, with bounds: returns dict dx, dres, dgamma,
    dbeta and their bounds.  Elements whose pre-activation lies within the forward's error bound of 0 have an undecided
    ReLU mask: they may count either way, so their |g| joins the bounds of the sums and their own dx / dres are exempt."""
    pre, xhat, invstd, M = r['pre'], r['xhat'], r['invstd'], r['M']
    N, C, H, W = pre.shape
    g = gy.double()
    if pool:
        g = F.interpolate(g, scale_factor=2, mode='nearest') / 4
        g = F.pad(g, (0, W - g.shape[3], 0, H - g.shape[2]))
    amb = torch.zeros_like(pre, dtype=torch.bool)
    ga_amb = torch.zeros_like(g)
    if relu:
        amb = pre.abs() <= fwd_c * r['fwd_abs']
        ga_amb = g.abs() * amb                                    # (|g| before the mask: it may count there or not)
        g = g * (pre > 0)
    v = lambda t: t.view(1, -1, 1, 1)
    dbeta = g.sum(dim=(0, 2, 3))
    dgamma = (g * xhat).sum(dim=(0, 2, 3))
    chain = bn_rows_per_thread(M, C, bf16) * U32
    ga = g.abs()
    xh_abs = xhat.abs() + v(invstd * r['mean'].abs())        # |xhat| and the float32 mean's rounding in it
    b_dbeta = chain * ga.sum(dim=(0, 2, 3)) + ga_amb.sum(dim=(0, 2, 3))
    b_dgamma = (chain + 4 * U32) * (ga * xh_abs).sum(dim=(0, 2, 3)) + (ga_amb * xhat.abs()).sum(dim=(0, 2, 3))
    gd = gamma.double()
    a = gd * invstd
    dx = v(a) * (g - v(dbeta / M) - xhat * v(dgamma / M))
    dx_abs = v(a.abs()) * (8 * U32 * (ga + v(dbeta.abs() / M) + xh_abs * v(dgamma.abs() / M))
                           + v(b_dbeta / M) + xhat.abs() * v(b_dgamma / M))
    out = dict(dx=dx, dres=g, dgamma=dgamma, dbeta=dbeta, b_dgamma=b_dgamma, b_dbeta=b_dbeta, exempt=amb)
    out['b_dx'] = (BF16_REL * dx.abs() if bf16 else 0) + dx_abs
    out['b_dres'] = (BF16_REL * g.abs() if bf16 else 0 * g) + 2 * U32 * ga
    return out


# ------------------------------------------------------------------------------------------------------------ GRU
def rnn_ref(rnn, x, gy, whh_round=None):
    """outputs and gradients of a batch_first nn.RNNBase (nn.GRU or nn.LSTM, one or two directions) evaluated in float64 on the
    CPU (a copy of `rnn`; W_hh optionally passed through whh_round first, e.g. a float16 rounding).
    -> (y, [dx] + [grad of every parameter])"""
    import copy
    g64 = copy.deepcopy(rnn).cpu().double()
    if whh_round is not None:
        with torch.no_grad():
            for n, p in g64.named_parameters():
                if n.startswith('weight_hh'):
                    p.copy_(whh_round(p))
    xr = x.detach().cpu().double().requires_grad_(True)
    y, _ = g64(xr)
    y.backward(gy.detach().cpu().double())
    return y.detach(), [xr.grad] + [p.grad for p in g64.parameters()]


gru_ref = rnn_ref


def _pool_input(N, Cn, H, W, g, kind):
    """bf16 channels-last input of the frequency max / mean + max pool tests, drawn on g's device: 'plain', 'ties' (exact zeros,
    repeated quarter values, all-zero columns, the w = 0 value repeated later on) or 'nan'"""
    DEV = g.device
    x = torch.randn((N, Cn, H, W), device=DEV, generator=g)
    if kind == 'ties':
        x = torch.relu(x).mul(4).round().div(4)                             # exact zeros and repeated quarter values
        x[:, ::5, :, :] = 0.0                                               # all-zero frequency columns
        x[:, 1::7, :, W // 2:] = x[:, 1::7, :, :1].expand(-1, -1, -1, W - W // 2)   # the w = 0 value repeated later on
    elif kind == 'nan':
        x[0, 3, 1, W - 2] = float('nan')
        x[0, 3, 1, W - 1] = float('nan')
        x[1 % N, 9, 0, 0] = float('nan')
    return x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
