"""GPU tests of the decay measurement (salsa_amd/csrc/rir_decay.hip through its C entry point salsa_rir_decay, salsa_amd/rooms.py:
rir_acoustics, calibrate_room) against the float64 reference of tests/decay_reference.py.

Shapes: response lengths 1, 2, both sides of the kernel's 256 threads, 7200 (a run of 29 taps per thread), the switch between the
kernel's two instantiations -- 8192 (a run of 32, LDS row stride 33: the last even run of the 33-dword rows), 8193 and 8448 (a run of
33: stride = run, rows that abut without a pad, at 8448 the last row ending at the array's end), 8449 (a run of 34: the first of the
65-dword rows) -- and both sides of the longest (runs of 64), each as a bank of 3 x 4 responses of twelve families (decay_reference.FAMILIES: geometric
and two-slope decays, silence, an impulse at either end, a decay cut to exact zeros inside the fit ranges, make_rir_bank noise tails,
image-source responses of the CPU path, a largest |h| that occurs twice); one channel and sixteen channels at one length each; one
bank of 2^31 + 262144 input floats.
Every output lies inside NaN guard bands, the input 4-byte aligned only.

Held (decay_reference.holds): the peak, the five crossings and the NaN / inf pattern exactly; the energy and the curve within L 2^-53
relative of the correctly rounded sums; the fitted times, headrooms, DRR and C50 within 4 Y + 1e-12 |reference|, Y the distance of the
reference's own float64 yardsticks (two other summation orders) from it.  Only cases whose knife-edge margin exceeds 1e-9 are used
(none of these is dropped; the helper allows one in ten).  A reference is computed once per shape and shared."""
import ctypes as C

import numpy as np
import pytest
import torch

import decay_reference as dr
from salsa_amd import _lib

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARD = 67                                                                     # elements on either side of every buffer: odd
LENGTHS = [1, 2, 255, 256, 257, 7200, 8192, 8193, 8448, 8449, 16383, 16384]
SIZE = (6.0, 5.0, 3.2)
MEASURED = """largest ratio (error) / Y per quantity over every kept case of every shape above, on one MI355X (the bound is 4 Y + 1e-12 |ref|)
  quantity       kernel    torch leg on the device (L = 7200 only)
  edt            2.00      1.00
  t20            2.00      1.00
  t30            1.00      0.12
  headroom_edt   3.00      1.00
  headroom_t20   2.00      0.50
  headroom_t30   0.50      0.17
  drr_db         1.00*     0.18
  c50_db         1.00      1.00
  (* and one case with Y = 0: image_source_y at L = 256, DRR 6.8999 dB, both yardsticks on the reference's very value, the kernel
  8.9e-16 = one ulp away; the floor of 6.9e-12 admits it.  The errors themselves: times and headrooms at most 10 ulp of the value
  (the largest error of a time is 1.4e-16 s), DRR and C50 at most 3.8e-15 dB, which is 272 ulp for a DRR of 0.079 dB.)
  the kernel at the switch between its instantiations (runs of 32, 33, 33, 34 taps; LDS row strides 33, 33, 33, 35), none above the table:
  L       edt    t20    t30    headroom_edt   headroom_t20   headroom_t30   drr_db   c50_db
  8192    0.50   0.60   0.11   1.00           0.50           0.12           0.26     1.00
  8193    1.00   0.60   0.25   1.00           2.00           0.17           0.20     0.00
  8448    1.00   1.00   0.17   1.00           1.00           0.22           0.15     0.11
  8449    0.43   1.50   0.12   0.50           1.00           0.22           0.15     1.00
  No case was dropped for its knife-edge margin.  energy and curve: within L 2^-53 everywhere.
  calibrate_room((6, 5, 3.2), 0.3) on the device: beta 0.8206 -> 0.7488 -> 0.7653 -> 0.7619, 4 evaluations, mean T20 0.298921 s by
  the kernel; the reference gives 0.298921 s on the device generator's responses and on the CPU generator's alike: the two generators'
  realised T20 differ by 2.2e-9 of the target."""


def _run(h, want_edc=True, fs=dr.FS, hw=None):
    """salsa_rir_decay on h (R, C, L) float32 -> params (R, C, 15), edc (R, C, L) or None, numpy; guard bands checked"""
    R, Cn, L = h.shape
    hw = dr.halfwidth(fs) if hw is None else hw
    lib = _lib.load()
    P = lib.salsa_rir_decay_params()
    src = torch.full((h.size + 2 * GUARD,), float('nan'), dtype=torch.float32, device=DEV)
    src[GUARD:GUARD + h.size] = torch.from_numpy(np.array(h, np.float32).reshape(-1)).to(DEV)
    n_p, n_e = R * Cn * P, R * Cn * L
    out = torch.full((n_p + 2 * GUARD,), float('nan'), dtype=torch.float64, device=DEV)
    out[GUARD:GUARD + n_p] = -7.0                                               # not NaN: an element the kernel leaves alone shows
    curve = torch.full((n_e + 2 * GUARD,), float('nan'), dtype=torch.float64, device=DEV)
    curve[GUARD:GUARD + n_e] = -7.0
    rc = lib.salsa_rir_decay(C.c_void_p(src[GUARD:].data_ptr()), R, Cn, L, fs, hw, C.c_void_p(out[GUARD:].data_ptr()),
                             C.c_void_p(curve[GUARD:].data_ptr()) if want_edc else None, C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    for buf, n in ((out, n_p), (curve, n_e)):
        assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all()), 'a guard band was written'
    params = out[GUARD:GUARD + n_p].view(R, Cn, P).cpu().numpy()
    assert not np.any(params == -7.0), 'a parameter was not written'
    body = curve[GUARD:GUARD + n_e].view(R, Cn, L).cpu().numpy()
    if not want_edc:
        assert np.all(body == -7.0), 'the curve was written though none was asked for'
        return params, None
    assert not np.any(body == -7.0) and not np.isnan(body).any(), 'a tap of the curve was not written'
    return params, body


def _report(what, ratios):
    print('WORST %s: %s' % (what, ', '.join('%s %.2f' % kv for kv in sorted(ratios.items()))))


# ---- the kernel against the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L', LENGTHS)
def test_kernel_against_the_reference(L):
    the_case = dr.case(L)
    params, edc = _run(the_case[1])
    _report('L = %d' % L, dr.holds('kernel', params, edc, the_case))
    assert np.all(np.diff(edc, axis=-1) <= 0), 'the curve never increases'
    assert np.array_equal(edc[..., 0].view(np.uint64), params[..., 0].view(np.uint64)), 'the energy is the curve at tap 0'


@pytest.mark.parametrize('shape', [(2, 1, 769), (1, 16, 513)])
def test_kernel_with_one_and_with_sixteen_channels(shape):
    R, Cn, L = shape
    the_case = dr.case(L, R, Cn, seed=3)
    params, edc = _run(the_case[1])
    _report('%d x %d x %d' % shape, dr.holds('kernel', params, edc, the_case))


def test_direct_halfwidth_and_fs_reach_the_kernel():
    """DRR with a direct path of one tap and of the whole response, C50 and the times at another sampling rate"""
    h = np.stack([dr.family(name, 3000, 5) for name in ('noise_tail', 'two_slope', 'image_source_w', 'double_peak')])[None]
    for fs, hw in ((dr.FS, 0), (dr.FS, 16384), (8000.0, 7)):
        params, _ = _run(h, fs=fs, hw=hw)
        for c in range(4):
            ref, Y, m = dr.measure_case(h[0, c], fs, hw)
            assert m > dr.MIN_MARGIN
            w, g = ref['params'], params[0, c]
            assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(np.isinf(g), np.isinf(w))
            fin = np.isfinite(w)
            assert np.all(np.abs(g[fin] - w[fin]) <= 4.0 * Y[fin] + 1e-12 * np.abs(w[fin])), (fs, hw, c)
        if hw == 16384:
            assert np.all(params[0, :, dr.IDX['drr_db']] == np.inf)


# ---- exact properties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L', [257, 7200, 8448, 8449, 16384])
def test_exact_properties(L):
    h = dr.case(L)[1]
    params, edc = _run(h)
    again, edc_again = _run(h)
    assert np.array_equal(params.view(np.uint64), again.view(np.uint64)) and np.array_equal(edc.view(np.uint64), edc_again.view(np.uint64)), \
        'two calls give equal bits'
    alone, edc_alone = _run(h[1:2])
    assert np.array_equal(alone[0].view(np.uint64), params[1].view(np.uint64)) and np.array_equal(edc_alone[0].view(np.uint64), edc[1].view(np.uint64)), \
        'a response alone gives the bits it has in a batch'
    without, none = _run(h, want_edc=False)
    assert none is None and np.array_equal(without.view(np.uint64), params.view(np.uint64)), 'the parameters do not depend on the curve\'s store'


def test_offsets_past_two_to_the_31():
    """8193 responses x 16 channels x 16384 taps = 2^31 + 262144 input floats (8.6 GB), no curve: the last response's offset rc x L does
    not fit 32 bits.  All are silent but the last, which carries the families: its parameters are those of the same response measured
    alone, bit for bit; every silent response gives energy 0, peak 0 and NaN elsewhere."""
    R, Cn, L = 8193, 16, 16384
    n = R * Cn * L
    assert n == (1 << 31) + 262144
    free = torch.cuda.mem_get_info()[0]
    assert free > 10 * 2 ** 30, 'this test wants 10 GB of device memory'
    lib = _lib.load()
    P = lib.salsa_rir_decay_params()
    _, h = dr.bank(L, 1, Cn)
    src = torch.full((n + 2 * GUARD,), float('nan'), dtype=torch.float32, device=DEV)
    src[GUARD:GUARD + n].zero_()
    src[GUARD + n - Cn * L:GUARD + n] = torch.from_numpy(h.reshape(-1)).to(DEV)
    n_p = R * Cn * P
    out = torch.full((n_p + 2 * GUARD,), float('nan'), dtype=torch.float64, device=DEV)
    out[GUARD:GUARD + n_p] = -7.0
    rc = lib.salsa_rir_decay(C.c_void_p(src[GUARD:].data_ptr()), R, Cn, L, dr.FS, dr.halfwidth(), C.c_void_p(out[GUARD:].data_ptr()), None,
                             C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[:GUARD]).all()) and bool(torch.isnan(out[GUARD + n_p:]).all()), 'a guard band was written'
    params = out[GUARD:GUARD + n_p].view(R, Cn, P).cpu().numpy()
    del src, out
    torch.cuda.empty_cache()
    assert not np.any(params == -7.0), 'a parameter was not written'
    silent, zero = params[:-1], [dr.IDX['energy'], dr.IDX['peak']]
    assert not silent[..., zero].view(np.uint64).any(), 'a silent response has energy +0.0 and peak +0.0'
    assert np.isnan(np.delete(silent, zero, axis=-1)).all(), 'a silent response has NaN elsewhere'
    alone, _ = _run(h, want_edc=False)
    assert np.array_equal(params[-1].view(np.uint64), alone[0].view(np.uint64)), 'the last response, past 2^31, is not what it is alone'
    assert np.isfinite(params[-1][:, dr.IDX['t20']]).sum() >= 8 and params[-1][:, dr.IDX['energy']].max() > 1.0


# ---- the public path -----------------------------------------------------------------------------------------------------------------
def test_rir_acoustics_runs_the_kernel_and_the_switch_leaves_it(monkeypatch):
    from salsa_amd import rooms, scenes as sc
    the_case = dr.case(7200)
    h = the_case[1]
    params, edc = _run(h)
    d_h = torch.from_numpy(np.array(h)).to(DEV)
    got = rooms.rir_acoustics(d_h, edc=True)                                   # a CUDA tensor is measured where it is
    assert np.array_equal(got.params.view(np.uint64), params.view(np.uint64)) and np.array_equal(got.edc.view(np.uint64), edc.view(np.uint64))
    assert np.array_equal(got.t20.view(np.uint64), params[..., dr.IDX['t20']].view(np.uint64)) and got.edc.shape == h.shape
    from_array = rooms.rir_acoustics(h, device=DEV)
    assert from_array.edc is None and np.array_equal(from_array.params.view(np.uint64), params.view(np.uint64))
    bank = sc.RirBank(h, [0, 90, 180], [0, 0, 0], 'foa')
    assert np.array_equal(bank.acoustics(device=DEV).params.view(np.uint64), params.view(np.uint64))
    monkeypatch.setattr(rooms, 'HIP_DECAY', False)                             # the composed torch path on the device: the same bounds
    leg = rooms.rir_acoustics(d_h, edc=True)
    monkeypatch.setattr(rooms, 'HIP_DECAY', True)
    _report('torch on the device', dr.holds('torch leg', leg.params, leg.edc, the_case))


def test_calibrate_room_on_the_device():
    """calibrate_room((6, 5, 3.2), 0.3) with the generator and the measurement on the GPU.  The room is then measured by the REFERENCE on
    responses of the CPU generator: within 1 % of the target plus the difference between the two generators' realised T20 (both by
    the reference), which is printed and recorded in MEASURED."""
    from salsa_amd import rooms
    target = 0.3
    room = rooms.calibrate_room(SIZE, target, device=DEV)
    cal = room.calibration
    assert cal['evaluations'] <= 6 and abs(cal['realised'] / target - 1) <= 0.01 and np.all(cal['headroom_db'] >= 15.0) and room.rt60 is None
    t20 = {}
    for where in ('cpu', DEV):
        h, _ = rooms.room_rirs('foa', room, cal['directions'], cal['distance'], cal['length'], device=where)
        t20[where] = float(np.mean([dr.measure(h[r, 0].cpu().numpy())['params'][dr.IDX['t20']] for r in range(h.shape[0])]))
    between = abs(t20['cpu'] - t20[DEV]) / target
    print('CALIBRATION beta %s, %d evaluations, realised %.6f s (kernel), reference on the device responses %.6f s, on the CPU responses %.6f s, '
          'generators differ by %.3e of the target' % ([round(float(b[0]), 4) for b in cal['beta_history']], cal['evaluations'], cal['realised'],
                                                        t20[DEV], t20['cpu'], between))
    assert abs(t20[DEV] - cal['realised']) <= 1e-9 * target                    # the kernel's mean is the reference's on the same responses
    assert abs(t20['cpu'] / target - 1) <= 0.01 + between
