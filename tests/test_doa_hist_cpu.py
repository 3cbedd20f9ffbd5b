"""The DOA histogram on the CPU: the conventions of the directional channels on plane waves through the oracle's
features, two sources disjoint in frequency, SALSA-Lite, the composed torch path against the float64 reference of
tests/doa_hist_reference.py on the built vote sets (the GPU test's list), and the refusals -- the launcher's without a device."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import doa_hist_reference as ref
from oracle import oracle as orc
from salsa_amd import _lib
from salsa_amd import localize as lz
from salsa_amd import scenes as sc

DIRECTIONS = ((30, 10), (-120, -40), (170, 60))
CASES = [('foa', 7, 2, 5), ('foa', 7, 1, 15), ('foa', 7, 4, 5), ('foa', 7, 1, 5), ('foa', 7, 2, 15), ('foa', 7, 4, 15),
         ('mic', 7, 2, 5), ('mic', 7, 1, 15), ('mic', 7, 4, 5), ('mic', 10, 2, 5), ('mic', 10, 4, 15)]


def make_localizer(fmt, K, step, **kw):
    return lz.DoaHistogram(audio_format=fmt, fmax_doa=9000 if fmt == 'foa' else 4000, max_sources=K, grid_step=step, **kw)


@functools.lru_cache(maxsize=None)
def built(fmt, n_channels, K, step):
    """(localizer, [features], [reference]) of one case, computed once and shared (tests/test_doa_hist_gpu.py reads it too)"""
    loc = make_localizer(fmt, K, step)
    assert (loc.col0, loc.col1) == ((0, 191) if fmt == 'foa' else (0, 33))
    xs = ref.build_features(loc, n_channels=n_channels)
    refs = [ref.reference(x, loc) for x in xs]
    for x in xs:
        x.setflags(write=False)
    return loc, xs, refs


def as_dict(res):
    r = res.numpy()
    return dict(count=r.count, n_votes=r.n_votes, cell=r.cell, score=r.score, direction=r.direction, spectrum=r.spectrum)


def _single(fmt, baffle, direction, feature_type='salsa'):
    length = 96 if baffle == 'rigid' else 40
    bank = sc.make_rir_bank(fmt, [direction], length, baffle=baffle)
    audio = ref.plane_wave_audio(bank, seed=abs(direction[0]))
    if feature_type == 'salsa_lite':
        feat = orc.extract_lite(audio, fmax_doa=2000)
        loc = lz.DoaHistogram(audio_format='mic', feature_type='salsa_lite', fmax_doa=2000)
    else:
        fmax = 9000 if fmt == 'foa' else 4000
        feat = orc.extract_salsa(audio, audio_format=fmt, fmax_doa=fmax)
        loc = lz.DoaHistogram(audio_format=fmt, fmax_doa=fmax)
    res = loc.localize(torch.from_numpy(feat[None]).contiguous()).numpy()
    return loc, feat, res


def _worst_single(res, direction):
    assert res.count.shape == (1, 20)
    assert np.all(res.count == 1), 'one peak in every label frame expected, got %s' % (res.count,)
    return float(ref.angle_deg(res.direction[0, :, 0], ref.unit(*direction)).max())


@pytest.mark.parametrize('fmt,baffle,key', [('foa', 'open', 'foa'), ('mic', 'open', 'mic_open'), ('mic', 'rigid', 'mic_rigid')])
def test_conventions_on_plane_waves(fmt, baffle, key):
    bound = ref.SINGLE_RIGID_BOUND_DEG if key == 'mic_rigid' else ref.SINGLE_BOUND_DEG[key]
    for d in DIRECTIONS:
        _, _, res = _single(fmt, baffle, d)
        worst = _worst_single(res, d)
        print('SINGLE %s %s worst %.3f deg' % (key, d, worst))
        assert worst <= bound, (key, d, worst)


def test_salsa_lite_single_source():
    for d in DIRECTIONS:
        _, _, res = _single('mic', 'open', d, feature_type='salsa_lite')
        worst = _worst_single(res, d)
        print('SINGLE lite %s worst %.3f deg' % (d, worst))
        assert worst <= ref.SINGLE_BOUND_DEG['lite'], (d, worst)


@pytest.mark.parametrize('fmt,bands', [('foa', ((200, 1500), (2000, 4000))), ('mic', ((100, 700), (900, 1500)))])
def test_two_sources_disjoint_in_frequency(fmt, bands):
    dirs = [(40, 0), (-100, 20)]
    bank = sc.make_rir_bank(fmt, dirs, 40)
    audio = ref.plane_wave_audio(bank, bands=bands, seed=7)
    fmax = 9000 if fmt == 'foa' else 4000
    feat = orc.extract_salsa(audio, audio_format=fmt, fmax_doa=fmax)
    loc = lz.DoaHistogram(audio_format=fmt, fmax_doa=fmax)
    res = loc.localize(torch.from_numpy(feat[None]).contiguous())
    r = res.numpy()
    assert np.all(r.count == 2), r.count
    rows = [np.array([(f, 0, k, az, el) for f in range(20) for k, (az, el) in enumerate(dirs)], np.int64)]
    err = lz.angular_errors(res, rows)
    print('TWO %s worst %.3f deg' % (fmt, err.errors.max()))
    assert err.missed == 0 and err.extra == 0 and len(err.errors) == 40 and err.errors.max() <= 3.0, (err.errors.max(), err.missed, err.extra)
    dcase = loc.rows(res)[0]
    assert dcase.shape == (40, 5) and np.all(dcase[:, 1] == 0) and set(dcase[:, 2]) == {0, 1}


@pytest.mark.parametrize('fmt,n_channels,K,step', CASES)
def test_torch_path_matches_the_float64_reference(fmt, n_channels, K, step):
    loc, xs, refs = built(fmt, n_channels, K, step)
    for x, r in zip(xs, refs):
        ref.check_margins(r)                                # the condition: no frame of the built inputs is excluded
        got = as_dict(loc.localize(torch.from_numpy(x.copy()), spectrum=True))
        worst = ref.check_against(got, r, direction_tol=1e-5, what='torch %s' % ((fmt, n_channels, K, step),))
        print('TORCH %s %s' % ((fmt, n_channels, K, step), worst))
        assert np.all(got['cell'][got['cell'] < 0] == -1)


def test_built_frames_are_what_they_are_named():
    """the vote counts and the peaks the list promises, by the reference alone"""
    loc, xs, refs = built('foa', 7, 2, 5)
    names = ref.FRAME_NAMES
    votes = np.concatenate([r['n_votes'].reshape(-1) for r in refs])
    count = np.concatenate([r['count'].reshape(-1) for r in refs])
    for name, n in (('n0', 0), ('n1', 1), ('n255', 255), ('n256', 256), ('n257', 257), ('full', 1528), ('dirty', 40)):
        assert votes[names.index(name)] == n, (name, votes[names.index(name)])
    expect = {'n0': 0, 'n1': 0, 'north': 1, 'south': 1, 'seam': 1, 'apart29': 2, 'apart31': 2, 'above': 1, 'below': 0, 'two': 2, 'full': 2}
    for name, c in expect.items():
        assert count[names.index(name)] == c, (name, count[names.index(name)])
    cells = np.concatenate([r['cell'].reshape(-1, 2) for r in refs])
    assert cells[names.index('north'), 0] == loc.n_cells - 1 and cells[names.index('south'), 0] == 0


def test_grid_and_columns():
    az, el = lz.doa_grid(5)
    assert len(az) == 2522 and (az[0], el[0]) == (0, -90) and (az[-1], el[-1]) == (0, 90) and (az[1], el[1]) == (-180, -85)
    assert az[72] == 175 and el[73] == -80
    L = _lib.load()
    for s in range(1, 40):
        assert L.salsa_doa_hist_cells(s) == (len(lz.doa_grid(s)[0]) if s in lz.GRID_STEPS else 0)
    assert (lz.DoaHistogram('foa').col0, lz.DoaHistogram('foa').col1) == (0, 191)
    assert (lz.DoaHistogram('mic').col0, lz.DoaHistogram('mic').col1) == (0, 33)
    loc = lz.DoaHistogram('foa', fmin_hz=200, fmax_hz=1500)
    assert (loc.col0, loc.col1) == (4, 31)
    np.testing.assert_allclose(lz.mic_matrix() @ (sc.MIC_RADIUS * (sc._unit(*zip(*sc.MIC_DIRECTIONS))[1:] - sc._unit(*zip(*sc.MIC_DIRECTIONS))[:1])),
                               np.eye(3), atol=1e-12)


def test_refusals():
    with pytest.raises(ValueError):
        lz.DoaHistogram('mic', feature_type='salsa_ipd')
    with pytest.raises(ValueError):
        lz.DoaHistogram('foa', grid_step=7)
    with pytest.raises(ValueError):
        lz.DoaHistogram('foa', grid_step=45)
    with pytest.raises(ValueError):
        lz.DoaHistogram('foa', max_sources=9)
    with pytest.raises(ValueError):
        lz.DoaHistogram('foa', frames_per_label=22)         # 22 x 191 > 4096 cells per label frame
    with pytest.raises(ValueError):
        lz.DoaHistogram('foa', min_score=0.0)
    loc = lz.DoaHistogram('foa')
    good = torch.zeros((1, 7, 16, 200))
    assert loc.localize(good).count.shape == (1, 2)
    for bad in (good.double(), good[:, :, :, ::2], good.permute(0, 1, 3, 2), good[:, :6].contiguous(), good[:, :, :7].contiguous(),
                good[..., :100].contiguous(), good.numpy()):
        with pytest.raises(ValueError):
            loc.localize(bad)


def test_launcher_refuses_before_any_device_call():
    L = _lib.load()
    mv, ms, mc = C.c_int(), C.c_int(), C.c_int()
    assert L.salsa_doa_hist_limits(C.byref(mv), C.byref(ms), C.byref(mc)) == 256
    assert (mv.value, ms.value) == (lz.MAX_VOTES, lz.MAX_SOURCES) and mc.value >= len(lz.doa_grid(3)[0])
    assert L.salsa_doa_hist_limits(None, None, None) == 256
    sup = L.salsa_doa_hist_supported
    assert sup(7, 200, 0, 191, 8, 5, 2) == 1 and sup(10, 200, 0, 33, 8, 15, 8) == 1 and sup(7, 200, 0, 128, 32, 3, 1) == 1
    for args in ((6, 200, 0, 191, 8, 5, 2), (7, 200, 0, 201, 8, 5, 2), (7, 200, 5, 5, 8, 5, 2), (7, 200, -1, 5, 8, 5, 2),
                 (7, 200, 0, 191, 22, 5, 2), (7, 200, 0, 191, 0, 5, 2), (7, 200, 0, 191, 8, 7, 2), (7, 200, 0, 191, 8, 2, 2),
                 (7, 200, 0, 191, 8, 45, 2), (7, 200, 0, 191, 8, 5, 9), (7, 200, 0, 191, 8, 5, 0)):
        assert sup(*args) == 0, args
    p = C.c_void_p(4096)                                    # never dereferenced: every call below is refused on the host
    M = (C.c_float * 9)(*range(9))
    base = dict(feat=p, B=1, Cf=7, T=25, F=200, col0=0, col1=191, P=8, fmt=0, M=None, grid=p, step=5, c0=0.96, inv=29.0, cs=0.86,
                ms=8.0, lo=0.5, hi=2.0, K=2, count=p, votes=p, cell=p, score=p, direction=p, spectrum=None, stream=None)

    def call(**kw):
        a = dict(base, **kw)
        return L.salsa_doa_hist(*[a[k] for k in base])

    for kw in (dict(feat=None), dict(grid=None), dict(count=None), dict(votes=None), dict(cell=None), dict(score=None), dict(direction=None),
               dict(fmt=1), dict(fmt=2), dict(B=0), dict(T=7), dict(Cf=6), dict(col1=201), dict(col1=0), dict(P=22), dict(step=7), dict(K=9),
               dict(K=0), dict(c0=1.0), dict(inv=0.0), dict(cs=1.0), dict(ms=0.0), dict(lo=0.0), dict(hi=0.4), dict(hi=float('inf')),
               dict(ms=float('nan')), dict(B=1 << 30, T=64)):
        assert call(**kw) == -1, kw
        assert 'salsa_doa_hist' in _lib.last_error()
    assert call(fmt=1, M=M, feat=None) == -1
