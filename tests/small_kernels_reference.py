"""High-precision restatements, seeded input builders and the checks (with their bounds) for the small kernels beside the hot
path: salsa_nn_seld_loss / _bwd (csrc/nn_loss.hip), salsa_nn_colsum2 (csrc/nn_reduce.hip), salsa_scaler_accumulate, salsa_normalize_batch and
salsa_to_freq_major (csrc/feature_utils.hip).  numpy only, no torch: tests/test_small_kernels_gpu.py hands the kernels' outputs to
the check_* functions below, tests/test_small_kernels_cpu.py hands them a float32 emulation of the kernels' arithmetic on the SAME
inputs -- so what is shown to be satisfiable on the host is exactly what is asked of the device.

Every check_* function asserts and returns {quantity: worst error / bound}."""
import numpy as np

U = 2.0 ** -24                                  # float32 unit roundoff


def _ratio(err, bound):
    err, bound = float(err), float(bound)
    return 0.0 if err == 0.0 else (float('inf') if bound == 0.0 else err / bound)


def same_bits(a, b):
    """elementwise: identical bit patterns, or both NaN"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    iv = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return (a.view(iv) == b.view(iv)) | (np.isnan(a) & np.isnan(b))


def untouched_pattern(n, dtype=np.float32):
    """n values of a fixed bit pattern for memory a kernel must leave alone: quiet and signalling NaN payloads, -0.0, plain words"""
    if np.dtype(dtype).itemsize == 4:
        words = np.array([0x7FC00001, 0xFFC12345, 0x7F812345, 0x80000000, 0xA5A5A5A5, 0x00000001, 0x7F800000], np.uint32)
    else:
        words = np.array([0x7FF8000000000001, 0xFFF8123456789ABC, 0x7FF0000000012345, 0x8000000000000000, 0xA5A5A5A5A5A5A5A5],
                         np.uint64)
    return np.resize(words, n).view(dtype)


# ------------------------------------------------------------------------------------------------------------------- SELD loss
SELD_SHAPES = [(1, 1), (1, 12), (21, 1), (111, 14),   # smallest shapes, nc = 14
               (640, 12),                            # the shape of test_fused_seld_loss_matches_the_eager_loss
               (16384, 1),                           # 64 workgroups x 256 threads: exactly one trip of the grid-stride loop
               (16385, 1),                           # one thread takes a second trip
               (2560, 12),                           # two uneven trips
               (3200, 12)]                           # na + nb = 153 600 > 512 x 256: the backward's block cap
SELD_MASKS = ('random', 'on', 'one', 'off')
SELD_EXTREMES = (0.0, -0.0, 16.7, -16.7, 30.0, -30.0, 88.0, -88.0, 104.0, -104.0)   # expf(88) is finite, expf(104) is not
SELD_WEIGHTS = (0.3, 0.7)


def seld_inputs(rows, nc, mask='random', extreme=False):
    """-> dict(logit [rows][nc], doa [rows][3 nc], sed_gt, doa_gt) float32.  logit = 3 randn; extreme: 200 positions (or all, when
    there are fewer) overwritten cyclically with SELD_EXTREMES; doa holds a few exact hits on doa_gt."""
    rng = np.random.RandomState(1000 * SELD_MASKS.index(mask) + 100 * int(extreme) + rows % 977 + 31 * nc)
    n = rows * nc
    if mask == 'random':
        z = (rng.rand(rows, nc) < 0.2).astype(np.float32)
    elif mask == 'on':
        z = np.ones((rows, nc), np.float32)
    else:
        z = np.zeros((rows, nc), np.float32)
        if mask == 'one':
            z.flat[rng.randint(n)] = 1.0
    z3 = np.concatenate([z, z, z], axis=1)
    doa_gt = ((rng.rand(rows, 3 * nc) * 2 - 1) * z3).astype(np.float32)
    logit = (3.0 * rng.randn(rows, nc)).astype(np.float32)
    if extreme:
        pos = rng.permutation(n)[:200]
        logit.flat[pos] = np.resize(np.array(SELD_EXTREMES, np.float32), pos.size)
    doa = np.tanh(rng.randn(rows, 3 * nc)).astype(np.float32)
    hits = rng.permutation(3 * n)[:4]
    doa.flat[hits] = doa_gt.flat[hits]                         # sign(0) = 0 (mostly where the mask is off)
    on = np.flatnonzero(z3)
    if on.size > 3:                                            # ... and where it is on, when that does not empty the sum
        doa.flat[on[:2]] = doa_gt.flat[on[:2]]
    return dict(logit=logit, doa=doa, sed_gt=z, doa_gt=doa_gt)


def seld_loss64(logit, doa, sed_gt, doa_gt, w):
    """float64 restatement of the reg_xyz loss (reference models/interfaces.py:304-355) -> (loss, sed, doa_loss, g_logit, g_doa):
    sed = mean of max(x, 0) - x z + log1p(exp(-|x|)); doa_loss = sum_k sum |p_k - t_k| m / sum m over the x | y | z blocks;
    g_logit = (sigmoid(x) - z) / n, g_doa = sign(e) z / sum m.  No active class anywhere: 0 / 0 = NaN, as the reference gives."""
    x, p, z, t = (np.asarray(a, np.float64) for a in (logit, doa, sed_gt, doa_gt))
    nc = z.shape[-1]
    assert x.shape == z.shape and p.shape == t.shape and p.shape[-1] == 3 * nc
    n = z.size
    sed = float(np.sum(np.maximum(x, 0.0) - x * z + np.log1p(np.exp(-np.abs(x)))) / n)
    z3 = np.concatenate([z, z, z], axis=-1)
    e = p - t
    m = np.float64(z.sum())
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        d = float(np.float64(np.sum(np.abs(e) * z3)) / m)
        g_doa = np.sign(e) * z3 / m
        g_logit = (1.0 / (1.0 + np.exp(-x)) - z) / n
    return float(w[0]) * sed + float(w[1]) * d, sed, d, g_logit, g_doa


def seld_g_doa32(inp):
    """what the kernel must write bit for bit: sign(e) z (float32(1) / float32(sum m)); sum m is an integer below 2^24, hence exact"""
    z3 = np.concatenate([inp['sed_gt']] * 3, axis=1)
    sign = (inp['doa'] > inp['doa_gt']).astype(np.float32) - (inp['doa'] < inp['doa_gt']).astype(np.float32)
    with np.errstate(invalid='ignore', divide='ignore'):
        inv_m = np.float32(1.0) / np.float32(inp['sed_gt'].sum(dtype=np.float64))
        return (sign * z3 * inv_m).astype(np.float32)


def seld_emulate32(inp, w):
    """the kernels' arithmetic in numpy float32 (per-element terms in float32, sums in float64, no contraction) -> (out3, g_logit, g_doa)"""
    x, z = inp['logit'], inp['sed_gt']
    n = x.size
    f32 = np.float32
    term = (np.maximum(x, f32(0)) - x * z) + np.log1p(np.exp(-np.abs(x)))
    assert term.dtype == np.float32
    z3 = np.concatenate([z, z, z], axis=1)
    ab = np.abs(inp['doa'] - inp['doa_gt']) * z3
    nc = z.shape[1]
    a = (ab[:, :nc] + ab[:, nc:2 * nc]) + ab[:, 2 * nc:]
    sed = f32(term.sum(dtype=np.float64) / n)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        d = f32(a.sum(dtype=np.float64)) / f32(z.sum(dtype=np.float64))
        loss = f32(w[0]) * sed + f32(w[1]) * d
        g_logit = (f32(1) / (f32(1) + np.exp(-x)) - z) * (f32(1) / f32(n))
    return np.array([loss, sed, d], np.float32), g_logit.astype(np.float32), seld_g_doa32(inp)


def check_seld(inp, w, out3, g_logit, g_doa):
    """The forward's bounds.
    sed: |sed - sed64| <= 2^-24 (3 mean|x| + 5): per term one rounding each for x z, the subtraction and the final addition, each at
      most |x| + 0.7 in size, expf and log1pf within 1 ulp, and the final cast.
    doa_loss: 1e-6 relative (three roundings per element, three in the division; test_accdoa_loss_kernel_against_float64's bound).
    loss: w_sed sed + w_doa d of the kernel's own two outputs, to 2 ulp.
    g_logit: 8 2^-24 / n (expf, 1 + e, the division, - z, 1 / n, the product).
    g_doa: bit-equal to seld_g_doa32.
    No active class: loss and doa_loss NaN, sed and g_logit as above."""
    out3, g_logit, g_doa = np.asarray(out3, np.float32), np.asarray(g_logit, np.float32), np.asarray(g_doa, np.float32)
    _, sed64, d64, gl64, _ = seld_loss64(inp['logit'], inp['doa'], inp['sed_gt'], inp['doa_gt'], w)
    x = inp['logit'].astype(np.float64)
    n = x.size
    r = {}
    assert np.isfinite(out3[1]) and np.isfinite(g_logit).all()
    r['sed'] = _ratio(abs(float(out3[1]) - sed64), U * (3.0 * np.abs(x).mean() + 5.0))
    r['g_logit'] = _ratio(np.abs(g_logit.astype(np.float64) - gl64).max(), 8.0 * U / n)
    if inp['sed_gt'].any():
        r['doa'] = _ratio(abs(float(out3[2]) - d64), 1e-6 * abs(d64))
        comb = float(np.float32(w[0])) * float(out3[1]) + float(np.float32(w[1])) * float(out3[2])
        r['loss'] = _ratio(abs(float(out3[0]) - comb), 2.0 * float(np.spacing(np.float32(abs(comb)))))
    else:
        assert np.isnan(d64) and np.isnan(out3[2]) and np.isnan(out3[0]), out3
    want = seld_g_doa32(inp)
    bad = int((~same_bits(g_doa.reshape(want.shape), want)).sum())
    assert bad == 0, 'g_doa: %d of %d elements differ from sign(e) z / sum(m)' % (bad, want.size)
    assert all(v <= 1.0 for v in r.values()), r
    return r


# ------------------------------------------------------------------------------------------------------------ SELD loss backward
BWD_SHAPES = [(640, 12), (3200, 12)]
BWD_WEIGHTS = [(0.3, 0.7), (0.0, 1.0)]
# the incoming gradients.  g_loss is a power of two so that g_loss * w is exact: the factor then carries ONE rounding (fused or
# not) and the product a second one, which is what the 2^-23 bound allows; all three are positive, so nothing cancels.
BWD_G = dict(g_loss=2.0, g_sed=0.37, g_doa=0.81)
BWD_COMBOS = [tuple(bool(i >> k & 1) for k in range(3)) for i in range(8)]          # (g_loss, g_sed, g_doa) present?


def bwd_inputs(rows, nc):
    """a [rows nc], b [rows 3 nc]: gradients of the size the forward leaves (about 1 / n), a few exact zeros and both signs"""
    rng = np.random.RandomState(rows + nc)
    a = (rng.randn(rows * nc) / (rows * nc)).astype(np.float32)
    b = (rng.randn(rows * 3 * nc) / (0.2 * rows * nc)).astype(np.float32)
    a[::97] = 0.0
    b[::89] = 0.0
    return a, b


def bwd_factors64(present, w):
    """(fa, fb) in float64 from the float32 scalars the kernel reads: fa = g_loss w_sed + g_sed, fb = g_loss w_doa + g_doa; absent = 0"""
    gl, gs, gd = (float(np.float32(BWD_G[k])) if p else 0.0 for k, p in zip(('g_loss', 'g_sed', 'g_doa'), present))
    return gl * float(np.float32(w[0])) + gs, gl * float(np.float32(w[1])) + gd


def bwd_emulate32(a, b, present, w):
    f32 = np.float32
    gl, gs, gd = (f32(BWD_G[k]) if p else f32(0) for k, p in zip(('g_loss', 'g_sed', 'g_doa'), present))
    return a * f32(gl * f32(w[0]) + gs), b * f32(gl * f32(w[1]) + gd)


def check_bwd(a, b, present, w, out_a, out_b):
    """out_a = a fa, out_b = b fb to 2^-23 relative (the compiler may fuse g_loss w + g: not bit-equal); a factor that is exactly
    zero gives exact zeros"""
    r = {}
    for name, x, f, out in (('out_a', a, bwd_factors64(present, w)[0], out_a), ('out_b', b, bwd_factors64(present, w)[1], out_b)):
        out = np.asarray(out, np.float32).reshape(x.shape)
        ref = x.astype(np.float64) * f
        if f == 0.0:
            assert not out.any(), '%s: factor 0 must give exact zeros' % name
            r[name] = 0.0
            continue
        err, bound = np.abs(out.astype(np.float64) - ref), 2.0 ** -23 * np.abs(ref)
        assert (err <= bound).all(), (name, present, w, float((err - bound).max()))
        nz = bound > 0
        r[name] = float((err[nz] / bound[nz]).max())
    return r


# --------------------------------------------------------------------------------------------------------------------- colsum2
# M in {1, 3, 4, 5, 16, 17, 63, 64, 65, 200, 4800} (the 16-row unrolled loop, its stride-4 tail, one and many row blocks of 64)
# x C in {1, 63, 64, 65, 768} (the col < C edge, one and many column blocks), pruned; every value of each is kept
COLSUM_PAIRS = [(1, 1), (1, 64), (3, 63), (3, 768), (4, 65), (5, 1), (5, 768), (16, 64), (17, 1), (17, 65), (63, 63), (64, 64),
                (64, 768), (65, 63), (65, 65), (200, 1), (200, 65), (200, 768), (4800, 1), (4800, 64), (4800, 65)]


def colsum_inputs(M, C, which=0):
    """[M][C] float32, each row scaled by 10^k, k in [-3, 2]; `which` selects one of two different matrices"""
    rng = np.random.RandomState(7 * M + C + 100003 * which)
    return (rng.randn(M, C) * 10.0 ** rng.randint(-3, 3, size=(M, 1))).astype(np.float32)


def colsum64(x):
    return np.asarray(x, np.longdouble).sum(axis=0).astype(np.float64)


def colsum_bound(x, pre=None):
    """per column (ceil(M / 64) + 18) 2^-24 sum_r |x[r, c]| (+ |pre|): the longest chain of float32 additions a value goes through is
    16 in a lane (in fact at most 8: the loop adds four rows as (v0 + v1) + (v2 + v3)), 2 across the four row lanes, and one
    atomic -- or one ordered slab addition and the final +=, whose first terms are exact -- per block of 64 rows"""
    s = np.abs(np.asarray(x, np.float64)).sum(axis=0)
    if pre is not None:
        s = s + np.abs(np.asarray(pre, np.float64))
    return (-(-x.shape[0] // 64) + 18) * U * s


def colsum_emulate32(x):
    """plain sequential float32 summation down the rows"""
    acc = np.zeros(x.shape[1], np.float32)
    for row in x:
        acc = acc + row
    return acc


def check_colsum(x, out, pre=None):
    ref = colsum64(x) + (0.0 if pre is None else np.asarray(pre, np.float64))
    err, bound = np.abs(np.asarray(out, np.float64) - ref), colsum_bound(x, pre)
    assert (err <= bound).all(), (x.shape, float((err - bound).max()))
    return {'colsum': float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0}


# ----------------------------------------------------------------------------------------------------------- scaler / normalise
# (B, C, T, F, n_sc): T < 64, T % 64 != 0, F > 256 (the second trip of the frequency loop; SALSA-Lite at n_fft 1024 has F = 382),
# F = 513 (a third trip), n_sc = C and n_sc < C
SCALER_SHAPES = [(1, 4, 1, 1, 1), (1, 4, 63, 64, 4), (2, 7, 64, 200, 4), (3, 7, 65, 257, 4), (2, 7, 130, 382, 4), (1, 10, 70, 513, 10),
                 (2, 10, 129, 128, 10), (1, 7, 200, 256, 7)]
NORMALIZE_SHAPES = SCALER_SHAPES + [(1, 4, 3, 65, 1), (3, 7, 5, 30, 4)]              # + row counts B n_sc T not divisible by 4


def scaler_inputs(B, C, T, F, n_sc):
    """-80 + 0.01 randn: the common offset turns an accidental float32 accumulation into an error near 1e-3 of sum|v| relative to
    the bound; channels >= n_sc hold NaN, so a read of them shows in the sums"""
    rng = np.random.RandomState(B + 3 * C + 5 * T + 7 * F + 11 * n_sc)
    feat = np.full((B, C, T, F), np.nan, np.float32)
    feat[:, :n_sc] = (-80.0 + 0.01 * rng.randn(B, n_sc, T, F)).astype(np.float32)
    return feat


def scaler_sums64(feat, n_sc):
    """[2][n_sc][F] float64: sum and sum of squares over clips and frames of the first n_sc channels (extended precision inside, so
    that this reference's own error is far below the bound)"""
    v = np.asarray(feat)[:, :n_sc].astype(np.longdouble)
    return np.stack([v.sum(axis=(0, 2)), (v * v).sum(axis=(0, 2))]).astype(np.float64)


def scaler_bound(feat, n_sc, calls=1):
    """1e-12 sum|v| per sum and 1e-12 sum v^2 per sum of squares: n 2^-53 for n <= 8192 float64 additions per entry"""
    v = np.abs(np.asarray(feat)[:, :n_sc].astype(np.float64))
    assert calls * v.shape[0] * v.shape[2] <= 8192
    return 1e-12 * calls * np.stack([v.sum(axis=(0, 2)), (v * v).sum(axis=(0, 2))])


def scaler_finish64(feat, n_sc):
    """(mean, std) [n_sc][F] float64 of the first n_sc channels, two passes, population variance"""
    v = np.asarray(feat)[:, :n_sc].astype(np.longdouble)
    mean = v.mean(axis=(0, 2))
    var = ((v - mean[None, :, None, :]) ** 2).mean(axis=(0, 2))
    return mean.astype(np.float64), np.sqrt(var).astype(np.float64)


def check_scaler(feat, n_sc, sums, calls=1):
    ref, bound = calls * scaler_sums64(feat, n_sc), scaler_bound(feat, n_sc, calls)
    sums = np.asarray(sums, np.float64).reshape(ref.shape)
    assert np.isfinite(sums).all(), 'a channel >= n_sc was read (NaN in the sums)'
    err = np.abs(sums - ref)
    assert (err <= bound).all(), (feat.shape, calls, float((err / bound).max()))
    return {'sum': float((err[0] / bound[0]).max()), 'sumsq': float((err[1] / bound[1]).max())}


def normalize_inputs(B, C, T, F, n_sc):
    """-> feat [B][C][T][F], mean, std [n_sc][F] float32; std in [0.5, 15]; channels >= n_sc hold untouched_pattern"""
    rng = np.random.RandomState(2 * B + 3 * C + 5 * T + 7 * F + 13 * n_sc)
    feat = untouched_pattern(B * C * T * F).reshape(B, C, T, F).copy()
    feat[:, :n_sc] = (-40.0 + 12.0 * rng.randn(B, n_sc, T, F)).astype(np.float32)
    mean = (-40.0 + 3.0 * rng.randn(n_sc, F)).astype(np.float32)
    std = rng.uniform(0.5, 15.0, size=(n_sc, F)).astype(np.float32)
    return feat, mean, std


def normalize32(feat, mean, std, n_sc):
    """the reference's own float32 arithmetic (dataset/database.py:197-202): feature[:n_sc] = (feature[:n_sc] - mean) / std"""
    out = np.array(feat, np.float32, copy=True)
    F = out.shape[-1]
    out[:, :n_sc] = (out[:, :n_sc] - mean.reshape(1, n_sc, 1, F)) / std.reshape(1, n_sc, 1, F)
    assert out.dtype == np.float32
    return out


# ---------------------------------------------------------------------------------------------------------------- to_freq_major
# rows in {1, 3} x T in {1, 63, 64, 65, 129} x F in {1, 63, 64, 65, 200, 382}, pruned; every value of each is kept
TRANSPOSE_SHAPES = [(1, 1, 1), (1, 1, 382), (3, 129, 1), (1, 63, 64), (1, 64, 63), (1, 64, 64), (3, 65, 65), (1, 65, 63), (3, 63, 200),
                    (1, 129, 200), (3, 64, 382), (1, 65, 382), (3, 129, 65)]


def transpose_inputs(rows, T, F):
    """every element distinct enough to show a misplaced one, with +-0, +-inf, NaN, the largest and smallest normal values and
    subnormals strewn in"""
    rng = np.random.RandomState(rows + 3 * T + 5 * F)
    x = rng.randn(rows, T, F).astype(np.float32)
    fi = np.finfo(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, fi.max, -fi.max, fi.tiny, -fi.tiny, fi.tiny / 4, -fi.tiny / 1024, 1e-45],
                       np.float32)
    pos = rng.permutation(x.size)[:max(1, x.size // 5)]
    x.flat[pos] = np.resize(special, pos.size)
    return x


def to_freq_major64(x):
    return np.ascontiguousarray(np.asarray(x).swapaxes(-1, -2).astype(np.float64))
