"""CPU side of tests/test_small_kernels_gpu.py (no GPU calls): the float64 restatements of tests/small_kernels_reference.py agree
with what is already pinned to the reference (the eager loss of salsa_amd/crnn/loss.py, which test_crnn_cpu.py holds to fixture g16,
and g21's scaler file); a float32 emulation of each kernel's arithmetic, on every input set the GPU file uses, stays inside the bound
the GPU file applies -- the bounds are satisfiable, and the printed shares say how much room they leave; and the five launchers
refuse bad arguments before any device call."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import small_kernels_reference as sk
from conftest import load_golden


@pytest.fixture(scope='module')
def lib():
    from salsa_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------- the restatements against what is pinned
class _Keep64:
    """stands in for a prediction tensor: seld_loss's .float() hands back the float64 tensor, so its eager lines run in float64"""

    def __init__(self, t):
        self.t = t

    def float(self):
        return self.t


@pytest.mark.parametrize('rows,nc,mask,extreme', [(111, 14, 'random', False), (640, 12, 'random', True), (21, 1, 'on', False),
                                                  (1, 12, 'one', True), (2560, 12, 'random', False)])
def test_seld_loss64_agrees_with_the_eager_loss_in_float64(rows, nc, mask, extreme):
    from salsa_amd.crnn import loss as L
    inp = sk.seld_inputs(rows, nc, mask, extreme)
    t = {k: torch.from_numpy(v.astype(np.float64)) for k, v in inp.items()}
    logit, doa = t['logit'].requires_grad_(True), t['doa'].requires_grad_(True)
    pred = {'event_frame_logit': _Keep64(logit), 'doa_frame_output': _Keep64(doa)}
    out = L.seld_loss(pred, t['sed_gt'], t['doa_gt'], sk.SELD_WEIGHTS)                      # CPU tensors: the eager lines
    assert all(o.dtype == torch.float64 for o in out)
    ref = sk.seld_loss64(inp['logit'], inp['doa'], inp['sed_gt'], inp['doa_gt'], sk.SELD_WEIGHTS)
    for name, a, b in zip(('loss', 'sed', 'doa'), out, ref[:3]):
        assert abs(float(a.detach()) - b) <= 1e-12 * abs(b), (name, float(a.detach()), b)
    g_logit, = torch.autograd.grad(out[1], logit, retain_graph=True)
    g_doa, = torch.autograd.grad(out[2], doa)
    for name, a, b in (('g_logit', g_logit.numpy(), ref[3]), ('g_doa', g_doa.numpy(), ref[4])):
        err = np.abs(a - b.reshape(a.shape))
        assert err.max() <= 1e-12 * np.abs(b).max(), (name, float(err.max()))


def test_seld_loss64_gives_nan_without_an_active_class():
    inp = sk.seld_inputs(21, 1, 'off')
    loss, sed, d, g_logit, g_doa = sk.seld_loss64(inp['logit'], inp['doa'], inp['sed_gt'], inp['doa_gt'], sk.SELD_WEIGHTS)
    assert np.isnan(loss) and np.isnan(d) and np.isfinite(sed) and np.isfinite(g_logit).all() and np.isnan(g_doa).all()


def test_scaler_sums64_reproduces_the_scaler_file_of_g21():
    """the sums of g21's two dev feature files, finished with scaler_finish's formula, give the reference's scaler file (same
    tolerance as test_scaler_math_reproduces_g21: the file is float32, and std comes from a variance of 9 frames)"""
    meta, a = load_golden('g21_baseline')
    seen = 0
    for t in meta['trees']:
        pre = 'tree_%s|%s|' % (t['format'], t['feature_type'])
        feats = [a[k] for k in sorted(a) if k.startswith(pre) and '_dev|' in k and k.endswith('|feature')]
        assert len(feats) == 2
        n_sc, F = feats[0].shape[0], feats[0].shape[2]
        sums = sum(sk.scaler_sums64(f[None], n_sc) for f in feats)
        n = sum(f.shape[1] for f in feats)
        mean = sums[0] / n
        std = np.sqrt(np.maximum(sums[1] / n - mean * mean, 0.0))                       # extractor.scaler_finish
        for name, got in (('mean', mean), ('std', std)):
            ref = a[[k for k in a if k.startswith(pre) and k.endswith('_feature_scaler.h5|' + name)][0]]
            assert ref.shape == (n_sc, 1, F)
            np.testing.assert_allclose(got.astype(np.float32), ref[:, 0], rtol=2e-6, atol=1e-6, err_msg=name)
            seen += 1
    assert seen >= 2


def test_normalize32_and_to_freq_major64_are_the_plain_expressions():
    feat, mean, std = sk.normalize_inputs(3, 7, 5, 30, 4)
    out = sk.normalize32(feat, mean, std, 4)
    for b, c, t in ((0, 0, 0), (2, 3, 4), (1, 2, 3)):
        assert np.array_equal(out[b, c, t], (feat[b, c, t] - mean[c]) / std[c])
    assert sk.same_bits(out[:, 4:], feat[:, 4:]).all() and np.isnan(feat[:, 4:]).any() and np.isfinite(out[:, :4]).all()
    x = sk.transpose_inputs(3, 65, 65)
    y = sk.to_freq_major64(x)
    assert y.shape == (3, 65, 65) and y.dtype == np.float64 and np.isnan(y).sum() == np.isnan(x).sum()
    assert np.array_equal(y[2, :, 64], x[2, 64, :].astype(np.float64), equal_nan=True)
    assert (np.abs(x[np.isfinite(x) & (x != 0)]) < np.finfo(np.float32).tiny).any()              # subnormals are in


# ----------------------------------------------------------------------------------------------- the bounds leave a correct kernel room
def test_the_gpu_bounds_hold_for_a_float32_emulation_on_every_gpu_input_set():
    worst = {}

    def note(kernel, r):
        for k, v in r.items():
            worst[kernel + ' ' + k] = max(worst.get(kernel + ' ' + k, 0.0), v)
    for rows, nc in sk.SELD_SHAPES:
        for mask in sk.SELD_MASKS:
            for extreme in (False, True):
                inp = sk.seld_inputs(rows, nc, mask, extreme)
                note('seld_loss', sk.check_seld(inp, sk.SELD_WEIGHTS, *sk.seld_emulate32(inp, sk.SELD_WEIGHTS)))
    for rows, nc in sk.BWD_SHAPES:
        a, b = sk.bwd_inputs(rows, nc)
        for w in sk.BWD_WEIGHTS:
            for present in sk.BWD_COMBOS:
                note('seld_loss_bwd', sk.check_bwd(a, b, present, w, *sk.bwd_emulate32(a, b, present, w)))
    for M, Cn in sk.COLSUM_PAIRS:
        for which in (0, 1):
            x = sk.colsum_inputs(M, Cn, which)
            note('colsum2', sk.check_colsum(x, sk.colsum_emulate32(x)))
    for shape in sk.SCALER_SHAPES:
        feat = sk.scaler_inputs(*shape)
        plain = np.stack([feat[:, :shape[4]].astype(np.float64).sum(axis=(0, 2)),
                          (feat[:, :shape[4]].astype(np.float64) ** 2).sum(axis=(0, 2))])        # float64, numpy's own order
        note('scaler_accumulate', sk.check_scaler(feat, shape[4], plain))
        note('scaler_accumulate twice', sk.check_scaler(feat, shape[4], plain + plain, calls=2))
    for k in sorted(worst):
        print('float32 emulation, %-32s: %5.1f %% of the bound' % (k, 100.0 * worst[k]))
    assert all(v <= 1.0 for v in worst.values())


def test_the_checks_reject_small_realistic_bugs():
    """the power of the checks themselves: each of these wrong results is what a plausible kernel bug produces"""
    inp = sk.seld_inputs(640, 12, 'random', True)
    w = sk.SELD_WEIGHTS
    out3, gl, gd = sk.seld_emulate32(inp, w)
    sk.check_seld(inp, w, out3, gl, gd)
    with pytest.raises(AssertionError):
        sk.check_seld(inp, w, out3, gl * np.float32(1 + 2e-6), gd)
    gd2 = gd.copy()
    gd2[0, 0] = -gd2[0, 0] if gd2[0, 0] != 0 else 1.0
    with pytest.raises(AssertionError):
        sk.check_seld(inp, w, out3, gl, gd2)
    short = {k: v[:600] for k, v in inp.items()}                                                 # a loop that stops early
    with pytest.raises(AssertionError):
        sk.check_seld(inp, w, sk.seld_emulate32(short, w)[0], gl, gd)
    x = sk.colsum_inputs(200, 65)
    with pytest.raises(AssertionError):
        sk.check_colsum(x, sk.colsum_emulate32(x[:199]))
    with pytest.raises(AssertionError):
        sk.check_colsum(x, sk.colsum_emulate32(sk.colsum_inputs(200, 65, 1)))
    feat = sk.scaler_inputs(2, 7, 130, 382, 4)
    f32 = np.stack([feat[:, :4].sum(axis=(0, 2), dtype=np.float32), (feat[:, :4] ** 2).sum(axis=(0, 2), dtype=np.float32)])
    with pytest.raises(AssertionError):
        sk.check_scaler(feat, 4, f32.astype(np.float64))                                         # float32 accumulators
    with pytest.raises(AssertionError):
        sk.check_scaler(feat, 5, np.zeros((2, 5, 382)) + np.nan)                                 # a read of channel 4


# ------------------------------------------------------------------------------------------------------------------ refusals
P = C.c_void_p(0x1000)          # stands in for a pointer: every call below is refused before anything reads it or touches a device
S = None                        # the null stream


def test_seld_loss_refuses_null_pointers_and_empty_shapes(lib):
    ok = [P, P, P, P, 8, 12, 0.3, 0.7, P, P, P, P, S]
    for i in (0, 1, 2, 3, 8, 9, 10, 11):
        assert lib.salsa_nn_seld_loss(*[None if k == i else a for k, a in enumerate(ok)]) == -1, i
    for i, bad in ((4, 0), (4, -1), (5, 0), (5, -3)):
        assert lib.salsa_nn_seld_loss(*[bad if k == i else a for k, a in enumerate(ok)]) == -1, (i, bad)


def test_seld_loss_bwd_refuses_null_pointers_and_empty_shapes(lib):
    ok = [P, 96, P, 288, None, None, None, 0.3, 0.7, P, P, S]
    for i in (0, 2, 9, 10):
        assert lib.salsa_nn_seld_loss_bwd(*[None if k == i else a for k, a in enumerate(ok)]) == -1, i
    for i, bad in ((1, 0), (1, -1), (3, 0), (3, -5)):
        assert lib.salsa_nn_seld_loss_bwd(*[bad if k == i else a for k, a in enumerate(ok)]) == -1, (i, bad)


def test_colsum2_refuses_bad_arguments_and_more_rows_than_its_grid_holds(lib):
    assert lib.salsa_nn_colsum2(None, None, P, None, 4, 4, S) == -1
    assert lib.salsa_nn_colsum2(P, None, None, None, 4, 4, S) == -1
    assert lib.salsa_nn_colsum2(P, P, P, None, 4, 4, S) == -1                  # a second matrix without its output
    for M, Cn in ((0, 4), (-1, 4), (4, 0), (4, -2)):
        assert lib.salsa_nn_colsum2(P, None, P, None, M, Cn, S) == -1, (M, Cn)
    for M in (65535 * 64 + 1, 1 << 40, (1 << 63) - 1):                         # ceil(M / 64) is grid y: at most 65535
        assert lib.salsa_nn_colsum2(P, None, P, None, M, 4, S) == -1, M
        assert lib.salsa_nn_colsum2(P, P, P, P, M, 4, S) == -1, M


def _einval(lib, rc, name):
    from salsa_amd import _lib
    assert rc == _lib.E_INVAL, (name, rc)
    assert name in _lib.last_error()


def test_scaler_accumulate_refuses_bad_arguments_and_what_its_grid_cannot_hold(lib):
    ok = [P, 2, 7, 64, 200, 4, P, S]                                           # feat, batch, channels, frames, freq, n_sc, sums
    for i in (0, 6):
        _einval(lib, lib.salsa_scaler_accumulate(*[None if k == i else a for k, a in enumerate(ok)]), 'salsa_scaler_accumulate')
    for i, bad in ((1, 0), (1, -1), (2, 0), (3, 0), (3, -1), (3, 2 ** 31 - 1), (4, 0), (4, -7), (5, 0), (5, -1), (5, 8)):
        _einval(lib, lib.salsa_scaler_accumulate(*[bad if k == i else a for k, a in enumerate(ok)]), 'salsa_scaler_accumulate')
    _einval(lib, lib.salsa_scaler_accumulate(P, 65536, 7, 64, 200, 4, P, S), 'salsa_scaler_accumulate')          # batch is grid z
    _einval(lib, lib.salsa_scaler_accumulate(P, 2 ** 31 - 1, 7, 64, 200, 4, P, S), 'salsa_scaler_accumulate')
    _einval(lib, lib.salsa_scaler_accumulate(P, 2, 65536, 64, 200, 65536, P, S), 'salsa_scaler_accumulate')      # n_sc is grid y
    _einval(lib, lib.salsa_scaler_accumulate(P, 2, 70000, 64, 200, 65536, P, S), 'salsa_scaler_accumulate')


def test_normalize_batch_refuses_bad_arguments(lib):
    ok = [P, 2, 7, 64, 200, 4, P, P, S]                                        # feat, batch, channels, frames, freq, n_sc, mean, std
    for i in (0, 6, 7):
        _einval(lib, lib.salsa_normalize_batch(*[None if k == i else a for k, a in enumerate(ok)]), 'salsa_normalize_batch')
    for i, bad in ((1, 0), (1, -1), (2, 0), (3, 0), (3, -1), (3, 2 ** 31 - 1), (4, 0), (4, -7), (5, 0), (5, -1), (5, 8)):
        _einval(lib, lib.salsa_normalize_batch(*[bad if k == i else a for k, a in enumerate(ok)]), 'salsa_normalize_batch')
    # (batch n_sc frames + 3) / 4 workgroups must stay below 2^31
    _einval(lib, lib.salsa_normalize_batch(P, 2 ** 31 - 1, 4, 8, 200, 1, P, P, S), 'salsa_normalize_batch')


def test_to_freq_major_refuses_bad_arguments(lib):
    ok = [P, 3, 65, 200, P, S]                                                 # feat, rows, frames, freq, out
    for i in (0, 4):
        _einval(lib, lib.salsa_to_freq_major(*[None if k == i else a for k, a in enumerate(ok)]), 'salsa_to_freq_major')
    for i, bad in ((1, 0), (1, -1), (1, 65536), (2, 0), (2, -1), (2, 65535 * 64 + 1), (3, 0), (3, -1)):
        _einval(lib, lib.salsa_to_freq_major(*[bad if k == i else a for k, a in enumerate(ok)]), 'salsa_to_freq_major')
