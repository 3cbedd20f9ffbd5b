"""CPU tests of the decay measurement and the room calibration (salsa_amd/rooms.py: rir_acoustics, calibrate_room; include/salsa_hip.h:
salsa_rir_decay): the float64 reference of tests/decay_reference.py against closed forms, the composed torch
path (device='cpu') against the reference with the bounds the GPU test holds the kernel to, the launcher's refusals (all of them come
before any device call, so they run without a GPU), the exports, and calibrate_room on the CPU path."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import decay_reference as dr
from conftest import ROOT

SIZE = (6.0, 5.0, 3.2)
LENGTHS = (1, 2, 255, 256, 257, 7200)


@pytest.fixture(scope='module')
def lib():
    from salsa_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ---- the reference against closed forms ------------------------------------------------------------------------------------------------
def test_reference_reproduces_the_geometric_decay_in_closed_form():
    """h[n] = r^n in float64, r = 10^(-3 / (T fs)), T = 0.3 s, L = 16384: EDC[n] = r^(2n) (1 - r^(2 (L - n))) / (1 - r^2); the curve is a
    straight line but for the cut's term, 10^-13.6 of the level at the start and 10^-10 at -35 dB, so every fit gives T to 1e-9."""
    L, T = 16384, 0.3
    h = dr.geometric(L, T, dtype=np.float64)
    got = dr.measure(h)
    closed = dr.geometric_edc(L, T)
    assert np.all(np.abs(got['edc'] - closed) <= 1e-12 * closed)
    p = got['params']
    print('EDT %.13f T20 %.13f T30 %.13f' % (p[dr.IDX['edt']], p[dr.IDX['t20']], p[dr.IDX['t30']]))
    for name in ('edt', 't20', 't30'):
        assert abs(p[dr.IDX[name]] / T - 1.0) < 1e-9, name
    assert p[dr.IDX['peak']] == 0 and p[dr.IDX['energy']] == got['edc'][0]
    r2 = 10.0 ** (-6.0 / (T * dr.FS))
    # i(x) = ceil(x / (-10 log10 r^2)) up to the cut's term; -5 dB falls on tap 600 exactly, where rounding decides: either is right
    per_tap = -10.0 * np.log10(r2)
    for k, x in enumerate(dr.LEVELS_DB[1:], 1):
        assert abs(p[dr.IDX['cross_0db'] + k] - (-x) / per_tap) <= 1.0
    # headroom: the slope times the taps left; DRR and C50: geometric series
    assert abs(p[dr.IDX['headroom_t20']] - per_tap * (L - 1 - p[dr.IDX['cross_25db']])) < 1e-6
    hw, early = dr.halfwidth(), 1200
    e_dir, e_all = (1 - r2 ** (hw + 1)) / (1 - r2), (1 - r2 ** L) / (1 - r2)
    assert abs(p[dr.IDX['drr_db']] - 10 * np.log10(e_dir / (e_all - e_dir))) < 1e-9
    e_early = (1 - r2 ** early) / (1 - r2)
    assert abs(p[dr.IDX['c50_db']] - 10 * np.log10(e_early / (e_all - e_early))) < 1e-9


def test_reference_edge_cases():
    nan, inf = float('nan'), float('inf')
    zero = dr.measure(np.zeros(100, np.float32))['params']
    assert zero[0] == 0 and zero[1] == 0 and np.all(np.isnan(zero[2:]))
    first = dr.measure(dr.impulse(100, 0))['params']
    assert first[dr.IDX['energy']] == 1 and first[dr.IDX['peak']] == 0 and np.all(np.isnan(first[2:8]))     # EDC[i(hi)] = 0: NaN, not -inf
    assert first[dr.IDX['drr_db']] == inf and first[dr.IDX['c50_db']] == inf and list(first[10:]) == [0, 1, 1, 1, 1]
    last = dr.measure(dr.impulse(100, 99, -0.5))['params']
    assert last[dr.IDX['energy']] == 0.25 and last[dr.IDX['peak']] == 99 and np.all(np.isnan(last[2:8])) and np.all(np.isnan(last[11:]))
    twice = dr.measure(dr.double_peak(300, 1))['params']
    assert twice[dr.IDX['peak']] == 5
    one = dr.measure(np.array([-2.0], np.float32))['params']
    assert one[0] == 4 and one[1] == 0 and np.all(np.isnan(one[2:8])) and one[8] == inf and one[9] == inf
    # the cut's bias at the end of a range, as the 15 dB rule states it: 10 log10(1 - 10^(-headroom / 10))
    assert abs(10 * np.log10(1 - 10 ** -1.5) + 0.14) < 0.005 and abs(10 * np.log10(1 - 10 ** -1.0) + 0.46) < 0.005


# ---- the torch path against the reference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L', LENGTHS)
def test_torch_path_against_the_reference_on_every_family(L):
    from salsa_amd import rooms
    the_case = dr.case(L)
    got = rooms.rir_acoustics(the_case[1], edc=True, device='cpu')
    assert got.params.shape == (3, 4, 15) and got.edc.shape == (3, 4, L) and got.edc.dtype == np.float64
    dr.holds('torch', got.params, got.edc, the_case)
    plain = rooms.rir_acoustics(the_case[1], device='cpu')
    assert plain.edc is None and np.array_equal(plain.params.view(np.uint64), got.params.view(np.uint64))
    for i, name in enumerate(dr.NAMES[:10]):
        assert np.array_equal(getattr(got, name).view(np.uint64), got.params[..., i].view(np.uint64)) and getattr(got, name).shape == (3, 4)
    for m in ('edt', 't20', 't30'):
        room = getattr(got, 'headroom_' + m)
        assert np.array_equal(got.truncated(m), ~(room >= 15.0)) and got.truncated(m).dtype == bool


def test_public_surface_on_banks_and_arguments():
    from salsa_amd import rooms, scenes as sc
    assert sc.rir_acoustics is rooms.rir_acoustics and sc.calibrate_room is rooms.calibrate_room and sc.RirAcoustics is rooms.RirAcoustics
    bank = sc.make_rir_bank('foa', [(0, 0), (90, 30)], 4800, rt60=0.2, seed=3)
    a = bank.acoustics(device='cpu')
    assert a.t20.shape == (2, 4) and np.all(np.abs(a.t20 / 0.2 - 1) < 0.1) and not a.truncated('t20').any()
    assert np.all(a.peak[:, 0] == 0) and np.all(a.drr_db[:, 0] > 6.0)                    # the 60 taps after the peak count as direct
    tap = bank.acoustics(device='cpu', direct_halfwidth=0)                              # make_rir_bank's own drr_db: a direct path of ONE tap
    assert np.allclose(tap.drr_db[:, 0], 6.0, atol=1e-5)
    # 0.083 s of a 0.3 s decay, 16.7 dB: the curve of the cut response still falls through -25 dB -- towards its own end -- so a fit
    # exists, reads short, and is flagged
    short = sc.make_rir_bank('foa', [(0, 0)], 2000, rt60=0.3, seed=3).acoustics(device='cpu')
    assert np.all(short.t20 < 0.27) and short.truncated('t20').all() and np.all(short.headroom_t20 < 5.0)
    import torch
    t = rooms.rir_acoustics(torch.from_numpy(bank.rirs), device='cpu')
    assert np.array_equal(t.params.view(np.uint64), a.params.view(np.uint64))
    for bad in (np.zeros((2, 4), np.float32), np.zeros((1, 17, 8), np.float32), np.zeros((1, 1, 16385), np.float32), np.zeros((1, 1, 0), np.float32)):
        with pytest.raises(ValueError):
            rooms.rir_acoustics(bad, device='cpu')
    with pytest.raises(ValueError):
        rooms.rir_acoustics(bank.rirs, fs=0, device='cpu')
    with pytest.raises(ValueError):
        rooms.rir_acoustics(bank.rirs, direct_halfwidth=-1, device='cpu')
    with pytest.raises(ValueError):
        a.truncated('t60')


# ---- the launcher -------------------------------------------------------------------------------------------------------------------------
def test_exports_and_the_parameter_enum(lib):
    from salsa_amd import _lib, rooms
    assert {'salsa_rir_decay', 'salsa_rir_decay_params'} <= set(_lib.EXPORTS)
    assert lib.salsa_rir_decay_params() == len(rooms.DECAY_PARAMS) == len(dr.NAMES) == 15
    hdr = open(os.path.join(ROOT, 'include', 'salsa_hip.h')).read()
    enum = dict((n.lower(), int(v)) for n, v in re.findall(r'SALSA_DECAY_(\w+) = (\d+)', hdr))
    assert enum.pop('params') == 15
    assert [n for n, _ in sorted(enum.items(), key=lambda kv: kv[1])] == list(rooms.DECAY_PARAMS) == list(dr.NAMES)
    i, d, vp = C.c_int, C.c_double, C.c_void_p
    assert list(lib.salsa_rir_decay.argtypes) == [vp, i, i, i, d, i, vp, vp, vp] and lib.salsa_rir_decay.restype is i
    src = open(os.path.join(ROOT, 'salsa_amd', 'csrc', 'rir_decay.hip')).read()
    assert src.index('#include "build_guard.h"') < src.index('#include <hip/hip_runtime.h>') and 'atomic' not in src.split('#include "build_guard.h"')[1]


def test_launcher_refuses_before_any_device_call(lib):
    """every refusal returns -1 with a message and touches no pointer: the pointers here are not addresses of anything"""
    from salsa_amd import _lib
    h, out, edc = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000)
    ok = dict(h=h, R=3, Cn=4, L=7200, fs=24000.0, hw=60, out=out)
    bad = [dict(h=None), dict(out=None), dict(R=0), dict(R=65536), dict(Cn=0), dict(Cn=17), dict(L=0), dict(L=16385), dict(fs=0.0),
           dict(fs=-24000.0), dict(fs=float('nan')), dict(fs=float('inf')), dict(hw=-1), dict(hw=16385)]
    for change in bad:
        a = dict(ok, **change)
        for curve in (edc, None):
            rc = lib.salsa_rir_decay(a['h'], a['R'], a['Cn'], a['L'], a['fs'], a['hw'], a['out'], curve, None)
            assert rc == _lib.E_INVAL, change
            assert _lib.last_error().startswith('salsa_rir_decay: '), change


# ---- calibration ----------------------------------------------------------------------------------------------------------------------------
def _remeasure(room, cal, device='cpu'):
    """the mean T20 of freshly generated probe responses (channel 0), measured by the REFERENCE"""
    from salsa_amd import rooms
    h, _ = rooms.room_rirs('foa', room, cal['directions'], cal['distance'], cal['length'], device=device)
    return float(np.mean([dr.measure(h[r, 0].cpu().numpy())['params'][dr.IDX['t20']] for r in range(h.shape[0])]))


@pytest.mark.parametrize('target', [0.2, 0.3])
def test_calibrate_room_reaches_the_target_on_the_cpu(target):
    from salsa_amd import rooms
    room = rooms.calibrate_room(SIZE, target, device='cpu')
    cal = room.calibration
    print('target %g: %d evaluations, beta %s, realised %.5f, probes %s' % (target, cal['evaluations'], [round(float(b[0]), 4) for b in cal['beta_history']],
                                                                         cal['realised'], np.round(cal['probes'], 4)))
    assert isinstance(room, rooms.ShoeboxRoom) and room.rt60 is None and np.array_equal(room.beta, cal['beta_history'][-1])
    assert cal['evaluations'] <= 6 and len(cal['beta_history']) == cal['evaluations'] and cal['measure'] == 't20' and cal['target'] == target
    assert abs(cal['realised'] / target - 1) <= 0.01 and cal['realised'] == cal['probes'].mean() and len(cal['probes']) == 4
    assert np.all(cal['headroom_db'] >= 15.0) and cal['length'] == int(np.ceil(target * 24000))
    assert abs(float(cal['beta_history'][0][0]) - rooms.eyring_beta(SIZE, target)) < 1e-15 and np.all(room.beta < cal['beta_history'][0])
    assert abs(_remeasure(room, cal) / target - 1) <= 0.01
    assert rooms.ShoeboxRoom(SIZE, rt60=target).calibration is None                    # a nominal room carries no record


def test_calibrate_room_keeps_an_absorption_ratio():
    from salsa_amd import rooms
    ratio = (1.0, 1.0, 2.0, 2.0, 4.0, 0.5)
    room = rooms.calibrate_room(SIZE, 0.2, absorption_ratio=ratio, device='cpu')
    cal = room.calibration
    assert cal['evaluations'] <= 6 and abs(cal['realised'] / 0.2 - 1) <= 0.01
    a = -np.log(room.beta)
    assert np.allclose(a / a[0], ratio, rtol=1e-12) and len(set(np.round(room.beta, 6))) == 4
    assert abs(_remeasure(room, cal) / 0.2 - 1) <= 0.01


def test_calibrate_room_raises():
    from salsa_amd import rooms
    with pytest.raises(ValueError, match='after 1 evaluations'):
        rooms.calibrate_room(SIZE, 0.3, max_iter=1, device='cpu')
    with pytest.raises(ValueError, match=r'headroom.*about 5072 taps would do'):       # the fits of the accepted step are truncated
        rooms.calibrate_room(SIZE, 0.3, length=3600, device='cpu')
    assert rooms.calibrate_room(SIZE, 0.3, length=5072, device='cpu').calibration['headroom_db'].min() >= 15.0     # ... and they do
    with pytest.raises(ValueError, match='reflection coefficient'):                    # Eyring's beta for 1e18 s rounds to 1: lossless
        rooms.calibrate_room(SIZE, 1e18, length=2400, device='cpu')
    for kw in (dict(measure='t60'), dict(absorption_ratio=(1, 1, 1, 1, 1, -1)), dict(absorption_ratio=(0,) * 6), dict(rtol=0)):
        with pytest.raises(ValueError):
            rooms.calibrate_room(SIZE, 0.3, device='cpu', **kw)
