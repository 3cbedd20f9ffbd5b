"""The decoder's Conformer blocks on the GPU: the three kernel families of salsa_amd/csrc/conformer.hip through
the C ABI against the float64 references of tests/conformer_reference.py, their structural properties (masks, NULL operands, bit
repeatability, batch invariance, tile edges), the block and decoder against the torch-operator path, and the whole model.

Bound of every comparison with float64: the kernel's maximum error may be at most 4 times the maximum error of the FLOAT32 evaluation
of the same reference on that case, plus one float32 ulp of the tensor's largest magnitude (4: another summation order, and the
device's exp / rsqrt against numpy's -- test_attn_gpu.py's factor and reason).  Where a result is a sum over more than 8 terms the
yardstick is the largest error of four float32 evaluations under different summation orders (_orders: the operands as they stand,
reversed, even then odd, one seeded shuffle; the second and fourth with the reference's sums taken left to right, the plain loop's
order, instead of numpy's pairwise one).  A row statistic of a tensor of one to five rows is a handful of numbers, and the ratio of
two such maxima exceeds any factor now and then (test_attn_gpu.py's note on its M = 1 case: 4.86); emulating the kernels' row mean
in numpy over 300 Gaussian rows, 1.5 % of single rows miss 4 x the pairwise yardstick alone and 0.3 % the left-to-right one alone.
Measured ratios are in MEASURED.

bias_swish_dropout takes C % 4 == 0 only, so a tensor's element count is a multiple of 4 and a hash pair is never cut by the tensor's
end: the pairing cannot meet a tail through this ABI.  The nearest cases are here instead: an odd number of float4 vectors (M odd, C 4)
and an odd number of rows."""
import ctypes as C

import numpy as np
import pytest
import torch

import conformer_reference as cr
from salsa_amd import _lib

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARD = 1024
FACTOR = 4.0
EPS = float(np.float32(1e-5))
TILE = 16                                                                     # SALSA_NN_CONV_MODULE_TILE; the backward's row tile is 8
MEASURED = """largest ratio (kernel error) / (float32-reference error) over every case of a family, per tensor, on one MI355X (2830 RATIO
lines of one run, all 42 tests passing in 15 s; 1.00: the kernel and the float32 evaluation round alike, element-wise results mostly):
  res_layernorm   z      y      mean    rstd   dx     dbranch  dgamma  dbeta
  gauss           1.00   1.00   1.96*   1.00   0.86   1.00     1.00    1.00
  constant        1.00   0.53   0.19    0.76   1.00   1.00     0.63    1.00
  offset (1e3)    1.00   0.79   0.79    1.00   0.84   1.00     0.79    1.00
  (* M = 1, C = 512, one row's mean: error 2.0e-8 against a yardstick of 1.0e-8.  The first run of this file, with numpy's pairwise
  sums in all four float32 evaluations, had this tensor at 11.6 on another row (1.2e-8 against 1.0e-9, floor 1.2e-10) and failed: the
  docstring above has the reason and what the evaluations are since.  No kernel was changed for it.)
  bias_swish_dropout   h 1.00   h without bias 1.00   da 1.00   db 1.25 (M 3, C 4096)
  conv_module     u      da     dw     dwb    dgamma  dbeta
  gauss           0.93   1.00   1.03   1.00   1.13    1.00
  impulse (3)     1.47   1.07   1.07   1.04   1.21    1.34       (1.47: impulse_mid, d 256, 3 taps, T 1)
  many tiles      0.55   0.74   0.37   0.41   0.58    0.55
  block, dropout off (HIP leg; yardsticks: the torch-operator leg and four numpy float32 evaluations): y 0.82, dx 0.73, parameters 1.25
  block, dropout 0.2 against the float64 reference fed the restated masks: y 0.99, dx 0.76, parameters 1.39 (norm_out.weight)
  decoder with two blocks (outputs and every parameter gradient, HIP blocks against the torch-operator leg): 2.57 (B 2, T' 40)
  Trainer.infer against the torch-operator leg: sed 1.00, doa 1.00 (both legs carry the bf16 encoder's and the half-weight GRU's error)
  No family needed more than 4."""


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _guarded(shape):
    """a NaN-filled buffer with the tensor in its middle -> (buffer, view)"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float('nan'), dtype=torch.float32, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _check_guards(*bufs):
    for buf, view in bufs:
        assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + view.numel():]).all()), 'a guard band was written'
        assert not bool(torch.isnan(view).any()), 'an output element was not written'


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if a is not None else None


def _holds(name, got, ref64, ref32, case):
    """ref32: one float32 evaluation, or a list of them (the yardstick is then their largest error)"""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref64).max()
    yard = max(np.abs(np.asarray(r, np.float64) - ref64).max() for r in (ref32 if isinstance(ref32, list) else [ref32]))
    floor = float(np.spacing(np.float32(np.abs(ref64).max())))
    print('RATIO %s %s err %.3e yard %.3e floor %.3e ratio %s' % (case, name, err, yard, floor, '%.2f' % (err / yard) if yard > 0 else '-'))
    assert np.isfinite(got).all(), (case, name)
    assert err <= FACTOR * yard + floor, '%s %s: error %.3e > %g x %.3e + %.3e' % (case, name, err, FACTOR, yard, floor)


def _eval32(n, fn):
    """fn() as float32 evaluation number n of four: odd ones with the reference's sums taken left to right"""
    if n & 1:
        with cr.sequential_sums():
            return fn()
    return fn()


def _orders(n, seed=0):
    """four orders of n things: as they stand, reversed, even then odd, one seeded shuffle"""
    i = np.arange(n)
    return [i, i[::-1].copy(), np.r_[i[0::2], i[1::2]], np.random.default_rng(n + seed).permutation(n)]


# ---- res_layernorm ------------------------------------------------------------------------------------------------------------------
def _run_res(x, branch, scale, p, seed, gamma, beta, dy, dz_in, want_z=True, want_y=True, want_dbranch=True):
    """the C ABI on numpy inputs, every output inside NaN guard bands -> dict of numpy results"""
    L = _lib.load()
    M, Cn = x.shape
    tx, tb, tg, tbt, tdy, tdz = (_dev(a) for a in (x, branch, gamma, beta, dy, dz_in))
    z, y, mean, rstd = (_guarded(s) for s in ((M, Cn), (M, Cn), (M,), (M,)))
    assert L.salsa_nn_res_layernorm_supported(M, Cn) == 1
    assert L.salsa_nn_res_layernorm_fwd(_ptr(tx), _ptr(tb), scale, p, seed, _ptr(tg) if want_y else None, _ptr(tbt) if want_y else None,
                                        _ptr(z[1]) if want_z else None, _ptr(y[1]) if want_y else None, _ptr(mean[1]) if want_y else None,
                                        _ptr(rstd[1]) if want_y else None, M, Cn, EPS, _stream()) == 0
    out = {}
    used = ([z] if want_z else []) + ([y, mean, rstd] if want_y else [])
    if dy is not None or dz_in is not None:
        dx, dbr, dgm, dbt = (_guarded(s) for s in ((M, Cn), (M, Cn), (Cn,), (Cn,)))
        ws_bytes = L.salsa_nn_res_layernorm_ws_bytes(M, Cn)
        assert ws_bytes > 0 and ws_bytes % 4 == 0
        ws = _guarded((ws_bytes // 4,))
        with_dy = dy is not None
        with_db = want_dbranch and branch is not None
        assert L.salsa_nn_res_layernorm_bwd(_ptr(tdy), _ptr(tdz), _ptr(tx), _ptr(tb), scale, p, seed, _ptr(tg) if with_dy else None,
                                            _ptr(mean[1]) if with_dy else None, _ptr(rstd[1]) if with_dy else None, _ptr(dx[1]),
                                            _ptr(dbr[1]) if with_db else None, _ptr(dgm[1]) if with_dy else None,
                                            _ptr(dbt[1]) if with_dy else None, _ptr(ws[1]) if with_dy else None, ws_bytes, M, Cn, _stream()) == 0
        used += [dx] + ([dbr] if with_db else []) + ([dgm, dbt, ws] if with_dy else [])
        out.update(dx=dx, **(dict(dbranch=dbr) if with_db else {}), **(dict(dgamma=dgm, dbeta=dbt) if with_dy else {}))
    torch.cuda.synchronize()
    _check_guards(*used)
    unused = [t for t in (z, y, mean, rstd) if not any(t is u for u in used)]
    assert all(bool(torch.isnan(t[0]).all()) for t in unused), 'an output that was not asked for was written'
    out.update(**(dict(z=z) if want_z else {}), **(dict(y=y, mean=mean, rstd=rstd) if want_y else {}))
    return {k: v[1].cpu().numpy() for k, v in out.items()}


def _res_case(family, M, Cn, seed):
    r = np.random.default_rng(seed)
    x, br = r.standard_normal((M, Cn)), r.standard_normal((M, Cn))
    br = np.sign(br) * (0.5 + np.abs(br))                                      # bounded away from 0: z == x only where the mask drops
    if family == 'constant':                                                   # zero variance without a branch: rstd = 1 / sqrt(eps)
        x[:] = r.standard_normal((M, 1))
    elif family == 'offset':                                                   # the cancellation case of E[z^2] - E[z]^2
        x += 1e3
    gamma, beta = 1.0 + 0.3 * r.standard_normal(Cn), r.standard_normal(Cn)
    dy, dz = r.standard_normal((M, Cn)), r.standard_normal((M, Cn))
    return tuple(a.astype(np.float32) for a in (x, br, gamma, beta, dy, dz))


def _res_reference(x, br, scale, mask, gamma, beta, dy, dz, dtype, rows=None, cols=None):
    """forward and backward of the reference, optionally with the rows and columns taken in another order (results in the natural one)"""
    if rows is not None:
        ir, ic = np.argsort(rows), np.argsort(cols)
        sub = lambda a: None if a is None else a[rows][:, cols]                # noqa: E731
        m = None if mask is None else (mask[0][rows][:, cols], mask[1])
        o = _res_reference(sub(x), sub(br), scale, m, gamma[cols], beta[cols], sub(dy), sub(dz), dtype)
        back = {'z': 2, 'y': 2, 'dx': 2, 'dbranch': 2, 'mean': 0, 'rstd': 0, 'dgamma': 1, 'dbeta': 1}
        return {k: (v[ir][:, ic] if back[k] == 2 else v[ir] if back[k] == 0 else v[ic]) for k, v in o.items()}
    z, y, mean, rstd = cr.res_layernorm_fwd(x, br, scale, mask, gamma, beta, EPS, dtype)
    dx, dbr, dg, db = cr.res_layernorm_bwd(dy, dz, x, br, scale, mask, gamma, mean, rstd, dtype)
    o = dict(z=z, y=y, mean=mean, rstd=rstd, dx=dx, dbranch=dbr, dgamma=dg, dbeta=db)
    return {k: v for k, v in o.items() if v is not None}


# (branch, z_out, y_out) x what the backward receives: every NULL combination of the forward, each with a backward it can be followed by
RES_COMBOS = [(True, True, True, 'both'), (True, False, True, 'dy'), (True, True, False, 'dz'), (False, True, True, 'both'),
              (False, False, True, 'dy'), (False, True, False, 'dz'), (True, True, True, 'dz'), (True, False, True, 'both')]
RES_DROPS = [(1.0, 0.0), (0.5, 0.2), (1.0, 0.2), (0.5, 0.0)]


@pytest.mark.parametrize('Cn', [256, 512])
@pytest.mark.parametrize('M', [1, 3, 4, 5, 257])
def test_res_layernorm_against_float64(M, Cn):
    n = 0
    for family in ('gauss', 'constant', 'offset'):
        x, br, gamma, beta, dy, dz = _res_case(family, M, Cn, 100 * M + Cn + len(family))
        for with_br, want_z, want_y, grads in RES_COMBOS:
            scale, p = RES_DROPS[n % 4]
            seed = cr.GPU_TEST_SEEDS[n % 2]
            n += 1
            b = br if with_br else None
            mask = cr.drop_mask((M, Cn), p, seed) if (with_br and p > 0) else None
            gdy, gdz = (dy if grads != 'dz' else None), (dz if grads != 'dy' else None)
            got = _run_res(x, b, scale, p, seed, gamma, beta, gdy, gdz, want_z, want_y)
            again = _run_res(x, b, scale, p, seed, gamma, beta, gdy, gdz, want_z, want_y)
            assert set(got) == set(again) and all(np.array_equal(got[k], again[k]) for k in got)            # two runs: equal bits
            if not want_y:                                                     # the backward had no dy: dx is dz_in, bit for bit
                assert np.array_equal(got['dx'], dz)
                if mask is not None:
                    assert np.array_equal(got['z'] == x, ~mask[0])
                continue
            f64 = _res_reference(x, b, scale, mask, gamma, beta, gdy, gdz, np.float64)
            f32 = [_eval32(i, lambda: _res_reference(x, b, scale, mask, gamma, beta, gdy, gdz, np.float32, rows, cols))
                   for i, (rows, cols) in enumerate(zip(_orders(M), _orders(Cn)))]
            case = 'res-%s M%d C%d br%d z%d %s scale%g p%g' % (family, M, Cn, with_br, want_z, grads, scale, p)
            for k in got:
                _holds(k, got[k], f64[k], [e[k] for e in f32], case)
            if mask is not None:
                if want_z:
                    assert np.array_equal(got['z'] == x, ~mask[0]), 'z == x exactly where the numpy mask drops and nowhere else'
                if gdz is not None:                                            # (dx has no zero of its own: dz_in is Gaussian)
                    assert np.array_equal(got['dbranch'] == 0, ~mask[0])
            if family == 'constant' and not with_br:
                np.testing.assert_allclose(got['rstd'], 1.0 / np.sqrt(EPS), rtol=1e-6)
                np.testing.assert_allclose(got['y'], np.broadcast_to(beta, (M, Cn)), rtol=0, atol=0)


@pytest.mark.parametrize('M,Cn', [(1, 256), (5, 512), (257, 256), (257, 512)])
def test_res_layernorm_is_add_layernorm_bit_for_bit_without_scale_and_dropout(M, Cn):
    L = _lib.load()
    for family in ('gauss', 'constant', 'offset'):
        x, br, gamma, beta, dy, _ = _res_case(family, M, Cn, 7 * M + Cn)
        got = _run_res(x, br, 1.0, 0.0, 0, gamma, beta, dy, None, want_z=False, want_dbranch=False)
        tx, tb, tg, tbt = (_dev(a) for a in (x, br, gamma, beta))
        y, mean, rstd = (_guarded(s) for s in ((M, Cn), (M,), (M,)))
        # (add_layernorm's first operand is the branch, its `res` the stream: x + res there is branch + x, the same sum)
        assert L.salsa_nn_add_layernorm_fwd(_ptr(tb), _ptr(tx), _ptr(tg), _ptr(tbt), _ptr(y[1]), _ptr(mean[1]), _ptr(rstd[1]), M, Cn, EPS, _stream()) == 0
        dx, dgm, dbt = (_guarded(s) for s in ((M, Cn), (Cn,), (Cn,)))
        ws_bytes = L.salsa_nn_add_layernorm_ws_bytes(M, Cn)
        ws = _guarded((ws_bytes // 4,))
        assert L.salsa_nn_add_layernorm_bwd(_ptr(_dev(dy)), _ptr(tb), _ptr(tx), _ptr(tg), _ptr(mean[1]), _ptr(rstd[1]), _ptr(dx[1]), _ptr(dgm[1]),
                                            _ptr(dbt[1]), _ptr(ws[1]), ws_bytes, M, Cn, _stream()) == 0
        torch.cuda.synchronize()
        for k, t in (('y', y), ('mean', mean), ('rstd', rstd), ('dx', dx), ('dgamma', dgm), ('dbeta', dbt)):
            assert np.array_equal(got[k], t[1].cpu().numpy()), (family, k)


# ---- bias + Swish + dropout ---------------------------------------------------------------------------------------------------------
def _run_bsd(a, b, dh, p, seed, want_db=True):
    L = _lib.load()
    M, Cn = a.shape
    ta, tb, td = _dev(a), _dev(b), _dev(dh)
    h, da, db = _guarded((M, Cn)), _guarded((M, Cn)), _guarded((Cn,))
    ws_bytes = L.salsa_nn_bias_swish_dropout_ws_bytes(M, Cn)
    assert ws_bytes > 0 and ws_bytes % 4 == 0 and L.salsa_nn_bias_swish_dropout_supported(M, Cn) == 1
    ws = _guarded((ws_bytes // 4,))
    assert L.salsa_nn_bias_swish_dropout_fwd(_ptr(ta), _ptr(tb), _ptr(h[1]), M, Cn, p, seed, _stream()) == 0
    assert L.salsa_nn_bias_swish_dropout_bwd(_ptr(td), _ptr(ta), _ptr(tb), _ptr(da[1]), _ptr(db[1]) if want_db else None,
                                             _ptr(ws[1]) if want_db else None, ws_bytes, M, Cn, p, seed, _stream()) == 0
    torch.cuda.synchronize()
    _check_guards(h, da, *([db, ws] if want_db else []))
    return tuple(t[1].cpu().numpy() for t in ((h, da, db) if want_db else (h, da)))


@pytest.mark.parametrize('Cn', [4, 1024, 4096])
@pytest.mark.parametrize('M', [1, 2, 3, 130])
def test_bias_swish_dropout_against_float64(M, Cn):
    r = np.random.default_rng(10 * M + Cn)
    b = r.standard_normal(Cn).astype(np.float32)
    v = r.standard_normal((M, Cn)) * 2
    v = (np.sign(v) * (0.1 + np.abs(v))).astype(np.float32)                    # |a + bias| >= 0.1: a zero output is a dropped element
    a = (v - b).astype(np.float32)
    assert (np.abs(a.astype(np.float64) + b) >= 0.0999).all()
    dh = r.standard_normal((M, Cn)).astype(np.float32)
    dh = np.where(dh == 0, np.float32(1), dh)
    for n, p in enumerate((0.0, 0.2, 0.5)):
        seed = cr.GPU_TEST_SEEDS[n % 2]
        mask = cr.drop_mask((M, Cn), p, seed) if p > 0 else None
        h, da, db = _run_bsd(a, b, dh, p, seed)
        again = _run_bsd(a, b, dh, p, seed)
        assert np.array_equal(h, again[0]) and np.array_equal(da, again[1]) and np.array_equal(db, again[2])   # db repeats bit for bit
        keep = np.ones((M, Cn), bool) if mask is None else mask[0]
        assert np.array_equal(h != 0, keep) and np.array_equal(da != 0, keep), 'the zero pattern is the numpy mask'
        case = 'bsd M%d C%d p%g' % (M, Cn, p)
        _holds('h', h, cr.bias_swish_dropout_fwd(a, b, mask), cr.bias_swish_dropout_fwd(a, b, mask, np.float32), case)
        da64, db64 = cr.bias_swish_dropout_bwd(dh, a, b, mask)
        f32 = []
        for i, rows in enumerate(_orders(M)):
            m = None if mask is None else (mask[0][rows], mask[1])
            f32.append(_eval32(i, lambda: cr.bias_swish_dropout_bwd(dh[rows], a[rows], b, m, np.float32)))
        _holds('da', da, da64, f32[0][0], case)
        _holds('db', db, db64, [e[1] for e in f32], case)
        if n == 1:                                                             # without dbias: the same h and da, nothing else written
            alone = _run_bsd(a, b, dh, p, seed, want_db=False)
            assert np.array_equal(alone[0], h) and np.array_equal(alone[1], da)
            pre = _run_bsd(v, None, dh, p, seed, want_db=False)                # bias NULL: a already holds it
            _holds('h-nobias', pre[0], cr.bias_swish_dropout_fwd(v, 0 * b, mask), cr.bias_swish_dropout_fwd(v, 0 * b, mask, np.float32), case)


# ---- convolution module -------------------------------------------------------------------------------------------------------------
def _run_conv(a, w, wb, gamma, beta, du):
    L = _lib.load()
    B, T, d2 = a.shape
    d, K = d2 // 2, w.shape[1]
    ta, tw, twb, tg, tb, tdu = (_dev(t) for t in (a, w, wb, gamma, beta, du))
    u, da, dw, dwb, dgm, dbt = (_guarded(s) for s in ((B, T, d), (B, T, 2 * d), (d, K), (d,), (d,), (d,)))
    assert L.salsa_nn_conv_module_supported(T, d, K) == 1
    ws_bytes = L.salsa_nn_conv_module_ws_bytes(B, T, d, K)
    assert ws_bytes > 0 and ws_bytes % 4 == 0
    ws = _guarded((ws_bytes // 4,))
    assert L.salsa_nn_conv_module_fwd(_ptr(ta), _ptr(tw), _ptr(twb), _ptr(tg), _ptr(tb), _ptr(u[1]), B, T, d, K, EPS, _stream()) == 0
    assert L.salsa_nn_conv_module_bwd(_ptr(tdu), _ptr(ta), _ptr(tw), _ptr(twb), _ptr(tg), _ptr(tb), _ptr(da[1]), _ptr(dw[1]), _ptr(dwb[1]),
                                      _ptr(dgm[1]), _ptr(dbt[1]), _ptr(ws[1]), ws_bytes, B, T, d, K, EPS, _stream()) == 0
    torch.cuda.synchronize()
    _check_guards(u, da, dw, dwb, dgm, dbt, ws)
    return tuple(t[1].cpu().numpy() for t in (u, da, dw, dwb, dgm, dbt))


CONV_NAMES = ('u', 'da', 'dw', 'dwb', 'dgamma', 'dbeta')


def _conv_case(family, B, T, d, K, seed):
    r = np.random.default_rng(seed)
    a = r.standard_normal((B, T, 2 * d))
    if family.startswith('impulse'):                                           # one non-zero row per sample: glu(0) = 0 everywhere else
        row = {'impulse_first': 0, 'impulse_last': T - 1, 'impulse_mid': T // 2}[family]
        keep = a[:, row].copy()
        a[:] = 0
        a[:, row] = 2 * keep
    w, wb = r.standard_normal((d, K)) / np.sqrt(K), 0.1 * r.standard_normal(d)
    gamma, beta, du = 1.0 + 0.3 * r.standard_normal(d), r.standard_normal(d), r.standard_normal((B, T, d))
    return tuple(t.astype(np.float32) for t in (a, w, wb, gamma, beta, du))


def _conv_references(a, w, wb, gamma, beta, du):
    """-> the float64 results and four float32 evaluations (channel orders of _orders, the taps summed from the last in two of them)"""
    d = w.shape[0]
    f64 = (cr.conv_module_fwd(a, w, wb, gamma, beta, EPS),) + cr.conv_module_bwd(du, a, w, wb, gamma, beta, EPS)
    f32 = []
    for n, c in enumerate(_orders(d)):
        ic, c2 = np.argsort(c), np.r_[c, d + c]
        args = (a[..., c2], w[c], wb[c], gamma[c], beta[c], EPS, np.float32, bool(n & 1))
        u = _eval32(n, lambda: cr.conv_module_fwd(*args))
        da, dw, dwb, dg, db = _eval32(n, lambda: cr.conv_module_bwd(du[..., c], *args))
        f32.append((u[..., ic], da[..., np.r_[ic, d + ic]], dw[ic], dwb[ic], dg[ic], db[ic]))
    return f64, f32


def _conv_times(K):
    bwd_tile = 8
    return sorted({1, 2, K // 2, K - 1, K, bwd_tile - 1, bwd_tile, bwd_tile + 1, TILE - 1, TILE, TILE + 1, 2 * bwd_tile + 3, 2 * TILE + 3, 130})


@pytest.mark.parametrize('K', [3, 7, 31])
@pytest.mark.parametrize('d', [256, 512])
def test_conv_module_against_float64_and_alone(d, K):
    """B = 3 against float64, and sample 1 of the batch alone (B = 1): u and da equal bit for bit -- no halo row leaks across samples"""
    for T in _conv_times(K):
        for n, family in enumerate(('gauss', 'impulse_first', 'impulse_last', 'impulse_mid')):
            if family != 'gauss' and T not in (1, 2, K // 2, K, TILE, TILE + 1, 2 * TILE + 3):
                continue
            case_in = _conv_case(family, 3, T, d, K, 1000 * T + d + K + n)
            got = _run_conv(*case_in)
            f64, f32 = _conv_references(*case_in)
            case = 'conv-%s d%d K%d T%d' % (family, d, K, T)
            for i, name in enumerate(CONV_NAMES):
                _holds(name, got[i], f64[i], [e[i] for e in f32], case)
            a, w, wb, gamma, beta, du = case_in
            alone = _run_conv(a[1:2], w, wb, gamma, beta, du[1:2])
            assert np.array_equal(alone[0], got[0][1:2]) and np.array_equal(alone[1], got[1][1:2]), case


@pytest.mark.parametrize('B,T,d,K', [(9, 130, 512, 31), (3, 350, 256, 3), (2, 512, 512, 7)])
def test_conv_module_many_tiles_per_workgroup_and_repeats(B, T, d, K):
    """more 8-row tiles than the backward's 128 workgroups (each walks several, restaging its LDS); the parameter gradients of two
    runs are equal bit for bit"""
    case_in = _conv_case('gauss', B, T, d, K, B + T + d + K)
    got, again = _run_conv(*case_in), _run_conv(*case_in)
    for a, b in zip(got, again):
        assert np.array_equal(a, b)
    f64, f32 = _conv_references(*case_in)
    for i, name in enumerate(CONV_NAMES):
        _holds(name, got[i], f64[i], [e[i] for e in f32], 'conv-many B%d T%d d%d K%d' % (B, T, d, K))


# ---- block and decoder --------------------------------------------------------------------------------------------------------------
D_AXIS0 = ('norm_ff1', 'norm_att', 'norm_conv', 'conv_norm', 'norm_ff2', 'norm_out', 'ff1_w2', 'ff2_w2', 'mha.out_proj', 'conv_dw', 'conv_p2')
D_AXIS1 = ('ff1_w1.weight', 'ff2_w1.weight', 'mha.in_proj_weight', 'conv_p1.weight', 'conv_p2.weight')


def _permute_block(P, c, inverse=False):
    """the block's parameters (or their gradients, inverse=True) with the model dimension taken in the order c"""
    d = len(c)
    c = np.argsort(c) if inverse else c
    out = {}
    for k, v in P.items():
        if k.rsplit('.', 1)[0] in D_AXIS0:
            v = v[c]
        if k.startswith('conv_p1.'):
            v = v[np.r_[c, d + c]]
        if k in D_AXIS1:
            v = v[:, c]
        out[k] = v
    return out


def _block_references(x, P, heads, masks, dy):
    """-> float64 (y, dx, G) and four float32 evaluations with the model dimension in the orders of _orders"""
    f64 = cr.block(x, P, heads, EPS, masks, dy)
    f32 = []
    for n, c in enumerate(_orders(x.shape[-1])):
        ic = np.argsort(c)
        m = {s: ((k[..., c], sc) if not s.endswith('_in') else (k, sc)) for s, (k, sc) in (masks or {}).items()}
        y, dx, G = _eval32(n, lambda: cr.block(x[..., c], _permute_block(P, c), heads, EPS, m, dy[..., c], np.float32))
        f32.append((y[..., ic], dx[..., ic], _permute_block(G, c, inverse=True)))
    return f64, f32


def _make_block(seed=3):
    from salsa_amd.crnn.model import ConformerBlock
    from salsa_amd.crnn.testing import seeded_fill
    blk = ConformerBlock(512)
    seeded_fill(blk, seed)
    return blk


@pytest.mark.parametrize('B,T', [(2, 40), (1, 65)])
def test_block_hip_against_torch_operators_and_float64(B, T, monkeypatch):
    """dropout off: the HIP leg must not reach F.layer_norm / F.silu / F.glu / nn.MultiheadAttention.forward; both legs against float64"""
    import torch.nn.functional as F
    from salsa_amd.crnn import conformer
    from salsa_amd.crnn.testing import dropout_off
    blk = _make_block().to(DEV).train()
    P = {k: v.cpu().numpy() for k, v in blk.state_dict().items()}
    r = np.random.default_rng(B * T)
    x, dy = r.standard_normal((B, T, 512)).astype(np.float32), r.standard_normal((B, T, 512)).astype(np.float32)
    real = {n: getattr(F, n) for n in ('layer_norm', 'silu', 'glu')}
    real_mha = torch.nn.MultiheadAttention.forward

    def leg(hip):
        monkeypatch.setattr(conformer, 'HIP_CONFORMER', hip)

        def refuse(*a, **k):
            raise AssertionError('a torch operator was reached with SALSA_HIP_CONFORMER=1')
        for n, f in real.items():
            monkeypatch.setattr(F, n, refuse if hip else f)
        monkeypatch.setattr(torch.nn.MultiheadAttention, 'forward', refuse if hip else real_mha)
        tx = _dev(x).requires_grad_(True)
        with dropout_off(blk):
            y = blk(tx)
            grads = torch.autograd.grad(y, [tx] + list(blk.parameters()), _dev(dy))
        return y.detach().cpu().numpy(), grads[0].cpu().numpy(), {k: g.cpu().numpy() for (k, _), g in zip(blk.named_parameters(), grads[1:])}

    hip, ref32 = leg(True), leg(False)
    (y64, dx64, G64), f32 = _block_references(x, P, 8, None, dy)
    case = 'block B%d T%d' % (B, T)
    _holds('y', hip[0], y64, [ref32[0]] + [e[0] for e in f32], case)
    _holds('dx', hip[1], dx64, [ref32[1]] + [e[1] for e in f32], case)
    for k in G64:
        _holds(k, hip[2][k], G64[k], [ref32[2][k]] + [e[2][k] for e in f32], case)


def test_block_with_dropout_against_float64_fed_the_restated_masks():
    from salsa_amd.crnn.conformer import draw_seed
    B, T, p = 2, 40, 0.2
    blk = _make_block(5).to(DEV).train()
    blk.drop.p = p
    P = {k: v.cpu().numpy() for k, v in blk.state_dict().items()}
    r = np.random.default_rng(11)
    x, dy = r.standard_normal((B, T, 512)).astype(np.float32), r.standard_normal((B, T, 512)).astype(np.float32)
    runs = []
    for _ in range(2):
        torch.manual_seed(cr.GPU_BLOCK_MANUAL_SEED)
        tx = _dev(x).requires_grad_(True)
        y = blk(tx)
        grads = torch.autograd.grad(y, [tx] + list(blk.parameters()), _dev(dy))
        runs.append((y.detach().cpu().numpy(), grads[0].cpu().numpy(), {k: g.cpu().numpy() for (k, _), g in zip(blk.named_parameters(), grads[1:])}))
    assert np.array_equal(runs[0][0], runs[1][0]) and all(np.array_equal(runs[0][2][k], runs[1][2][k]) for k in runs[0][2])
    torch.manual_seed(cr.GPU_BLOCK_MANUAL_SEED)
    seeds = [draw_seed(p) for _ in cr.SITES]
    masks = {s: cr.drop_mask((B, T, 1024 if s.endswith('_in') else 512), p, seed) for s, seed in zip(cr.SITES, seeds)}
    (y64, dx64, G64), f32 = _block_references(x, P, 8, masks, dy)
    assert np.abs(y64 - cr.block(x, P, 8, EPS, None)).max() > 0.01            # the masks matter
    got = runs[0]
    _holds('y', got[0], y64, [e[0] for e in f32], 'block-dropout')
    _holds('dx', got[1], dx64, [e[1] for e in f32], 'block-dropout')
    for k in G64:
        _holds(k, got[2][k], G64[k], [e[2][k] for e in f32], 'block-dropout')


_DECODER_REF = {}


def _decoder_case(B, Tp):
    """the decoder's input, loss weights, parameters and the float64 composition on the CPU (computed once per case)"""
    key = (B, Tp)
    if key not in _DECODER_REF:
        from salsa_amd.crnn.model import Decoder
        from salsa_amd.crnn.testing import seeded_fill
        g = torch.Generator().manual_seed(7 + Tp)
        dec = Decoder(512, 12, 256, 'bigru', 'avg', n_conformer_layers=2)
        seeded_fill(dec, 3)
        feat = torch.randn(B, 512, Tp, 12, generator=g).to(torch.bfloat16)
        w = (torch.randn(B, Tp, 12, generator=g), torch.randn(B, Tp, 36, generator=g))
        ref = Decoder(512, 12, 256, 'bigru', 'avg', n_conformer_layers=2).double()
        ref.load_state_dict({k: v.double() for k, v in dec.state_dict().items()})
        ref.eval()
        out = ref(feat.double())
        loss = (out['event_frame_logit'] * w[0].double()).sum() + (out['doa_frame_output'] * w[1].double()).sum()
        grads = torch.autograd.grad(loss, list(ref.parameters()))
        want = {'event': out['event_frame_logit'].detach().numpy(), 'doa': out['doa_frame_output'].detach().numpy()}
        want.update({k: g.numpy() for (k, _), g in zip(ref.named_parameters(), grads)})
        _DECODER_REF[key] = (dec.state_dict(), feat, w, want)
    return _DECODER_REF[key]


@pytest.mark.parametrize('B,Tp', [(2, 40), (1, 65)])
def test_decoder_hip_blocks_against_the_torch_path(B, Tp, monkeypatch):
    """Decoder(512, 12, 256, 'bigru', 'avg', n_conformer_layers=2) in training mode under dropout_off: the HIP blocks against the same
    decoder with SALSA_HIP_CONFORMER=0, both held to the float64 composition (the torch-path leg is the float32 yardstick)"""
    from salsa_amd.crnn import conformer
    from salsa_amd.crnn.model import Decoder
    from salsa_amd.crnn.testing import dropout_off
    sd, feat, w, want = _decoder_case(B, Tp)
    dec = Decoder(512, 12, 256, 'bigru', 'avg', n_conformer_layers=2)
    dec.load_state_dict(sd)
    dec = dec.to(DEV).train()
    x = feat.to(DEV).contiguous(memory_format=torch.channels_last)
    w = [t.to(DEV) for t in w]

    def leg(hip):
        monkeypatch.setattr(conformer, 'HIP_CONFORMER', hip)
        with dropout_off(dec):
            out = dec(x)
            loss = (out['event_frame_logit'] * w[0]).sum() + (out['doa_frame_output'] * w[1]).sum()
            grads = torch.autograd.grad(loss, list(dec.parameters()))
        got = {'event': out['event_frame_logit'].detach().cpu().numpy(), 'doa': out['doa_frame_output'].detach().cpu().numpy()}
        got.update({k: g.cpu().numpy() for (k, _), g in zip(dec.named_parameters(), grads)})
        return got

    hip, ref32 = leg(True), leg(False)
    for k in want:
        _holds(k, hip[k], want[k], ref32[k], 'decoder B%d T%d' % (B, Tp))


# ---- whole model --------------------------------------------------------------------------------------------------------------------
def test_trainer_bf16_steps_with_blocks_are_finite_move_and_repeat():
    from salsa_amd.crnn.train import Trainer, synthetic_batch
    x, sed, doa = synthetic_batch(4, DEV, seed=2, n_frames=128)
    runs = []
    for _ in range(2):
        tr = Trainer(DEV, total_steps=100, n_conformer_layers=2)
        named = {k: p for k, p in tr.raw_model.named_parameters() if '.conformer.' in k}
        before = {k: p.detach().clone() for k, p in named.items()}
        losses = [tr.train_step(x, sed, doa)[0] for _ in range(2)]
        runs.append(torch.stack(losses).cpu().numpy())
        assert len(named) == 60 and np.isfinite(runs[-1]).all()
        for k, p in named.items():
            assert not torch.equal(p.detach(), before[k]), k
    assert runs[0].tobytes() == runs[1].tobytes(), runs


def test_trainer_infer_equals_the_torch_operator_leg(monkeypatch):
    """Trainer.infer on (2, 7, 640, 200) under bf16 autocast: the encoder is the same kernels in both legs, so both decoders see the same
    bits; the float64 reference is the trainer's own decoder in double on the CPU, fed the encoder's output"""
    from salsa_amd.crnn import conformer
    from salsa_amd.crnn.model import Decoder
    from salsa_amd.crnn.train import Trainer
    tr = Trainer(DEV, n_conformer_layers=2)
    x = torch.randn(2, 7, 640, 200, generator=torch.Generator().manual_seed(1)).to(DEV)
    feats = []
    hook = tr.raw_model.encoder.register_forward_hook(lambda m, i, o: feats.append(o.detach().float().cpu()))
    legs = {}
    for hip in (True, False):
        monkeypatch.setattr(conformer, 'HIP_CONFORMER', hip)
        p, d = tr.infer(x)
        legs[hip] = (p.cpu().numpy(), d.cpu().numpy())
    hook.remove()
    assert torch.equal(feats[0], feats[1]) and legs[True][0].shape == (2, 80, 12) and legs[True][1].shape == (2, 80, 36)
    ref = Decoder(512, 12, 256, 'bigru', 'avg', n_conformer_layers=2).double().eval()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in tr.raw_model.decoder.state_dict().items()})
    with torch.no_grad():
        out = ref(feats[0].double())
    p64 = torch.sigmoid(out['event_frame_logit']).repeat_interleave(2, dim=1).numpy()
    d64 = out['doa_frame_output'].repeat_interleave(2, dim=1).numpy()
    _holds('sed', legs[True][0], p64, legs[False][0], 'infer')
    _holds('doa', legs[True][1], d64, legs[False][1], 'infer')


def test_tta_chunked_inference_both_decode_paths_and_scoring_with_blocks():
    """Trainer(n_conformer_layers=2) behind everything that sits on Trainer.infer: test-time augmentation (infer_tta), 320 / 200 test
    chunks, rows decoded on the host and on the device from one recorded forward, and the device's score of its rows against the
    host's rows as ground truth (the two round angles in float32 and float64: a degree apart at most, so every row is a hit)"""
    from salsa_amd.crnn.infer import infer_pipelined
    from salsa_amd.crnn.score import DeviceSeldScore, gt_rows_to_device
    from salsa_amd.crnn.train import Trainer
    torch.manual_seed(0)
    tr = Trainer(DEV, total_steps=10 ** 6, n_conformer_layers=2)
    feats = torch.randn(3, 7, 960, 200, generator=torch.Generator().manual_seed(9)).to(DEV)
    thr = float(torch.quantile(tr.infer_tta(feats[:1, :, :320], 'foa', 'salsa')[0].flatten(), 0.9))
    kw = dict(sub_batch=2, depth=2, n_label_frames=120, chunk_len=320, chunk_hop_len=200, eval_version='2020', sed_threshold=thr)
    tape = []

    def record(x):
        tape.append(tr.infer_tta(x, 'foa', 'salsa'))
        return tape[-1]
    host = infer_pipelined(3, lambda lo, hi: feats[lo:hi], record, decode='host', **kw)
    acc = DeviceSeldScore()
    dev = infer_pipelined(3, lambda lo, hi: feats[lo:hi], lambda x, it=iter(list(tape)): next(it), decode='device',
                          score=gt_rows_to_device(host, DEV) + (acc,), **kw)
    assert [len(r) for r in dev] == [len(r) for r in host] and sum(len(r) for r in host) > 100
    for a, b in zip(host, dev):
        for ra, rb in zip(a, b):
            assert tuple(ra[:2]) == tuple(rb[:2]) and all(abs(int(p) - int(q)) in (0, 1, 359) for p, q in zip(ra[2:], rb[2:])), (ra, rb)
    ER, F, LE, LR = (float(v) for v in acc.scores())
    assert F > 0.99 and LR > 0.99 and LE < 1.5 and ER < 0.01
