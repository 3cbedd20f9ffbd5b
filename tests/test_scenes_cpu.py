"""The scene renderer without a GPU: labels against the CSV readers, the seeded scene draw, the float32 yardstick
of tests/scene_reference.py, the exports and the launchers' refusals (decided before any device call), and the directions the synthetic
responses encode, read back by the CPU oracle from the float64 render."""
import ctypes as C
import os

import numpy as np
import pytest

import scene_reference as sr
from salsa_amd import _lib
from salsa_amd import scenes as sc
from salsa_amd.dataset import load_classwise_gt, load_trackwise_gt
from salsa_amd.synth import _ar1

HOP = 2400
NEW_EXPORTS = ('salsa_scene_rir_spectra_bytes', 'salsa_scene_rir_spectra', 'salsa_scene_workspace_bytes', 'salsa_scene_render')


def _pool(lengths, classes, seed=1):
    rng = np.random.RandomState(seed)
    return sc.EventPool([(0.1 * _ar1(rng.randn(n))).astype(np.float32) for n in lengths], classes)


def _bank(fmt='foa', length=64, **kw):
    return sc.make_rir_bank(fmt, [(70, -20), (-130, 40), (10, 0), (-50, 30)], length, **kw)


# ------------------------------------------------------------------------------------------------------------------ labels
def _label_scene():
    """20 label frames (N = 48000).  Events by index: 0 ends exactly on a frame boundary, 1 reaches one sample into the next frame,
    2 is short (for the last frame), 3 and 4 share class 5 and overlap on two tracks, 5 runs past the clip's end."""
    pool = _pool([2 * HOP - 100, 2 * HOP - 99, 7, 3 * HOP, 2 * HOP + 5, 4000], [0, 1, 2, 5, 5, 7])
    bank = _bank()
    items = [(0, 0, 100, 1.0, 0),            # [100, 4800): frames 0, 1 -- ends exactly on the boundary of frame 2
             (1, 1, 100 + 5 * HOP, 0.5, 1),  # [12100, 16801): frames 5, 6 and ONE sample of frame 7
             (3, 2, 9 * HOP + 17, 1.0, 0),   # class 5 on track 0: frames 9 .. 12
             (4, 3, 10 * HOP, 0.7, 1),       # class 5 on track 1: frames 10 .. 12 (same-class overlap, another direction)
             (2, 1, 19 * HOP + 2393, 1.0, 0),  # onset in the last frame, ends on the clip's last sample
             (5, 0, 48000 - 1000, 1.0, 1)]   # cut by the clip's end: frame 19 only
    return sc.Scenes.from_items(48000, [items], pool, bank), pool, bank


def test_rows_follow_the_dry_extent():
    scenes, pool, bank = _label_scene()
    rows = sc.scene_rows(scenes[0])
    assert rows.dtype == np.int64 and rows.shape[1] == 5
    frames = {i: sorted(r[0] for r in rows if (r[1], r[2]) == key) for i, key in enumerate([(0, 0), (1, 1), (5, 0), (5, 1), (2, 0), (7, 1)])}
    assert frames[0] == [0, 1] and frames[1] == [5, 6, 7] and frames[2] == [9, 10, 11, 12] and frames[3] == [10, 11, 12]
    assert frames[4] == [19] and frames[5] == [19]
    assert [tuple(r[3:]) for r in rows if r[0] == 0] == [(70, -20)]
    assert list(rows[:, 0]) == sorted(rows[:, 0])


@pytest.mark.parametrize('fmt', ['classwise', 'trackwise'])
def test_labels_equal_the_csv_readers_bit_for_bit(tmp_path, fmt):
    scenes, pool, bank = _label_scene()
    drawn = sc.draw_scenes(2, sc.synth_event_pool(12, 2, 3), bank, 8 * 24000, 11, max_polyphony=3, allow_same_class=True)
    for k, scene in enumerate([scenes[0], drawn[0], drawn[1]]):
        n_lab = scene.n_samples // HOP
        fn = str(tmp_path / ('meta%d.csv' % k))
        np.savetxt(fn, sc.scene_rows(scene), fmt='%d', delimiter=',')
        if fmt == 'classwise':
            want = load_classwise_gt(fn, 8 * n_lab, 12)
        else:
            want = load_trackwise_gt(fn, 8 * n_lab, 12)[:2]
        got = sc.scene_labels(scene, n_lab, 12, fmt)
        for g, w in zip(got, want):
            assert g.dtype == np.float32 and g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32))
        assert got[0].sum() > 0
    sed, doa = sc.scene_labels(scenes[0], 20, 12, fmt)
    if fmt == 'trackwise':                                                     # both tracks of class 5 are kept, in two slots
        assert sed[11, 5] == 1 and sed[11, 12 + 5] == 1 and sed[9, 12 + 5] == 0
    else:
        assert sed[11, 5] == 1 and sed[:, 5].sum() == 4
    assert sed[7, 1] == 1 and sed[2, 0] == 0 and sed[19, 2] == 1 and sed[19, 7] == 1
    empty = sc.Scenes.from_items(48000, [[]], pool, bank)
    sed, doa = sc.scene_labels(empty[0], 20, 12, fmt)
    assert sed.shape == (20, 12 * (3 if fmt == 'trackwise' else 1)) and not sed.any() and not doa.any() and doa.shape[1] == 3 * sed.shape[1]
    # rows at or past n_frames are dropped
    assert sc.scene_labels(scenes[0], 19, 12, fmt)[0].shape[0] == 19


def test_draw_is_seeded_and_keeps_its_promises():
    pool = sc.synth_event_pool(6, 3, 7)
    bank = _bank()
    N = 30 * 24000
    a, b = sc.draw_scenes(4, pool, bank, N, 5), sc.draw_scenes(4, pool, bank, N, 5)
    for f in sc.Scenes.FIELDS + ('clip_start',):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    other = sc.draw_scenes(4, pool, bank, N, 6)
    assert not (other.n_items == a.n_items and np.array_equal(other.onset, a.onset))
    assert a.n_items > 16 and np.all(a.onset + a.length <= N) and np.all(a.cls == pool.classes[a.event])
    assert np.all(a.azimuth == bank.azimuth[a.rir]) and np.all((a.gain <= 1.0) & (a.gain >= 10 ** (-12 / 20) * 0.999))
    for max_poly, same in ((1, False), (2, False), (3, False), (3, True)):
        s = sc.draw_scenes(3, pool, bank, N, 21, max_polyphony=max_poly, allow_same_class=same)
        seen_same = False
        for c in range(s.n_clips):
            rows = sc.scene_rows(s[c])
            per_frame = np.bincount(rows[:, 0], minlength=N // HOP)
            assert per_frame.max() <= max_poly and per_frame.max() >= min(max_poly, 2)
            cells = rows[:, 0] * 100 + rows[:, 1]
            dup = len(np.unique(cells)) != len(cells)
            seen_same = seen_same or dup
            assert same or not dup
        assert seen_same == same


# ------------------------------------------------------------------------------------------------------------------ yardstick
def test_float32_evaluations_land_near_and_not_on_float64():
    pool = _pool([700, 1500], [0, 1])
    bank = _bank(length=600, rt60=0.2, seed=4)
    scenes = sc.Scenes.from_items(4133, [[(0, 0, 17, 0.9, 0), (1, 2, 900, 0.4, 1), (0, 3, 3800, 1.0, 0)]], pool, bank)
    amb = (0.01 * np.random.RandomState(5).randn(1, 4, 4133)).astype(np.float32)
    ref = sr.render64(scenes, pool, bank, 4133, amb)
    assert ref.dtype == np.float64
    top, errs = sr.float32_yardstick(scenes, pool, bank, 4133, amb, ref)
    assert len(errs) == 4 and top == max(errs)
    for e in errs:
        assert 0 < e < 1e-5 * np.abs(ref).max()
    # the float64 restatement itself: against a direct sum at a few samples
    for c, n in ((0, 17), (2, 1000), (3, 4132), (1, 16)):
        want = float(amb[0, c, n])
        for e, r, o, g in sr._items(scenes, 0):
            s, h = pool.signals[e].astype(np.float64), bank.rirs[r, c].astype(np.float64)
            want += float(g) * sum(h[k] * s[n - o - k] for k in range(len(h)) if 0 <= n - o - k < len(s))
        assert abs(ref[0, c, n] - want) < 1e-12
    m = sr.support(scenes, pool, bank, 4133)
    assert m[0, 17] and not m[0, 16] and m[0, 4132] and m.shape == (1, 4133)
    assert np.array_equal(ref[0][:, ~m[0]], amb[0][:, ~m[0]].astype(np.float64))


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_exports_header_build_list_and_switch():
    text = open(os.path.join(_lib.INCLUDE_DIR, 'salsa_hip.h')).read()
    for name in NEW_EXPORTS:
        assert name + '(' in text and name in _lib.EXPORTS and hasattr(_lib.load(), name)
    assert _lib.PROTOTYPES['salsa_hip.h']['salsa_scene_workspace_bytes'] == (C.c_size_t, [C.c_int64, C.c_int, C.c_int])
    assert _lib.PROTOTYPES['salsa_hip.h']['salsa_scene_rir_spectra_bytes'][0] is C.c_size_t
    assert os.path.join(_lib.CSRC_DIR, 'scene_render.hip') in _lib.build_command()
    assert open(os.path.join(_lib.CSRC_DIR, 'scene_render.hip')).read().split('\n#include')[1].strip() == '"build_guard.h"'
    assert sc.HIP_SCENE is True or os.environ.get('SALSA_HIP_SCENE') == '0'
    assert 'SALSA_HIP_SCENE' in open(os.path.join(os.path.dirname(_lib.INCLUDE_DIR), 'README.md')).read()
    assert _lib.load().salsa_abi_version() == 2


def test_size_queries_give_their_stated_values():
    L = _lib.load()
    assert L.salsa_scene_rir_spectra_bytes(1, 1, 1) == 8192 + 4096
    assert L.salsa_scene_rir_spectra_bytes(3, 4, 512) == 8192 + 3 * 4 * 4096
    assert L.salsa_scene_rir_spectra_bytes(3, 4, 513) == 8192 + 3 * 4 * 2 * 4096
    assert L.salsa_scene_rir_spectra_bytes(2, 16, 16384) == 8192 + 2 * 16 * 32 * 4096
    for bad in ((0, 4, 100), (1, 0, 100), (1, 17, 100), (1, 4, 0), (1, 4, 16385), (-1, 4, 7)):
        assert L.salsa_scene_rir_spectra_bytes(*bad) == 0
    # items x min((max_len + 510) / 512 + 2, ceil(N / 512)) x 4096
    assert L.salsa_scene_workspace_bytes(1440000, 1, 1) == 2 * 4096
    assert L.salsa_scene_workspace_bytes(1440000, 2, 1) == 3 * 4096            # two samples can straddle a block edge: three input blocks
    assert L.salsa_scene_workspace_bytes(1440000, 513, 1) == 3 * 4096
    assert L.salsa_scene_workspace_bytes(1440000, 514, 1) == 4 * 4096
    assert L.salsa_scene_workspace_bytes(1440000, 72000, 960) == 960 * 143 * 4096
    assert L.salsa_scene_workspace_bytes(4133, 3000, 5) == 5 * 8 * 4096
    assert L.salsa_scene_workspace_bytes(4133, 100000, 5) == 5 * 9 * 4096      # never more blocks than the clip has
    assert L.salsa_scene_workspace_bytes(4133, 3000, 0) == 0
    for bad in ((0, 100, 1), (4133, 0, 1), (4133, 100, -1)):
        assert L.salsa_scene_workspace_bytes(*bad) == 0


def _render_args(**over):
    """a call that would be valid -- with HOST pointers everywhere, so that a launch with it would be an error"""
    n_items, n_clips = 3, 2
    a = dict(events=np.zeros(5000, np.float32), n_event_samples=5000, spectra=np.zeros(4096, np.float32), R=2, Cn=4, L=700,
             clip_start=np.array([0, 2, 3], np.int32), items=np.array([[0, 100, 4000], [0, 5, 4132], [100, 3000, 1000], [0, 1, 1]], np.int64),
             gains=np.ones(3, np.float32), n_clips=n_clips, n_items=n_items, max_len=3000, ambient=np.zeros(8, np.float32),
             out=np.zeros(8, np.float32), N=4133, ws=np.zeros(8, np.float32), ws_bytes=1 << 30)
    a.update(over)
    return a


def _render(a):
    p = lambda x: None if x is None else C.c_void_p(x.ctypes.data)
    return _lib.load().salsa_scene_render(p(a['events']), a['n_event_samples'], p(a['spectra']), a['R'], a['Cn'], a['L'], p(a['clip_start']),
                                          p(a['items']), p(a['gains']), p(a['clip_start']), p(a['items']), p(a['gains']), a['n_clips'],
                                          a['n_items'], a['max_len'], p(a['ambient']), p(a['out']), a['N'], p(a['ws']), a['ws_bytes'], None)


def _items_with(row, col, value):
    items = _render_args()['items'].copy()
    items[row, col] = value
    return items


BAD_RENDER = {
    'no events': dict(events=None), 'no spectra': dict(spectra=None), 'no clip_start': dict(clip_start=None), 'no items': dict(items=None),
    'no gains': dict(gains=None), 'no out': dict(out=None), 'no workspace': dict(ws=None),
    'no channel': dict(Cn=0), '17 channels': dict(Cn=17), 'no response': dict(R=0), 'rir length 0': dict(L=0), 'rir too long': dict(L=16385),
    'no clip': dict(n_clips=0), 'negative items': dict(n_items=-1), 'no sample': dict(N=0), 'event length 0': dict(max_len=0),
    'clip_start not from 0': dict(clip_start=np.array([1, 2, 3], np.int32)), 'clip_start not to n_items': dict(clip_start=np.array([0, 2, 2], np.int32)),
    'clip_start decreasing': dict(clip_start=np.array([0, 4, 3], np.int32)),
    'onset at N': dict(items=_items_with(1, 1, 4133)), 'onset negative': dict(items=_items_with(1, 0, -1)),
    'length 0': dict(items=_items_with(2, 0, 0)), 'length above the maximum': dict(items=_items_with(2, 1, 3001)),
    'event past the pool': dict(items=_items_with(0, 2, 4001)), 'event before the pool': dict(items=_items_with(0, 0, -1)),
    'rir index': dict(items=_items_with(3, 2, 2)), 'rir negative': dict(items=_items_with(3, 0, -1)),
    'gain not finite': dict(gains=np.array([1, np.inf, 1], np.float32)), 'gain nan': dict(gains=np.array([np.nan, 1, 1], np.float32)),
}


@pytest.mark.parametrize('what', sorted(BAD_RENDER))
def test_render_refuses_before_any_device_call(what):
    assert _render(_render_args(**BAD_RENDER[what])) == -1, what
    assert 'salsa_scene_render' in _lib.last_error()


def test_render_refuses_the_rest():
    many = 257
    a = _render_args(clip_start=np.array([0, many, many], np.int32), items=np.tile(_render_args()['items'][:, :1], (1, many)),
                     gains=np.ones(many, np.float32), n_items=many)
    assert _render(a) == -1 and '256' in _lib.last_error()                    # the stated cap on a clip's items
    need = _lib.load().salsa_scene_workspace_bytes(4133, 3000, 3)
    assert _render(_render_args(ws_bytes=need - 1)) == -5
    L = _lib.load()
    buf = np.zeros(4096, np.float32)
    p = C.c_void_p(buf.ctypes.data)
    for args in ((None, 2, 4, 700, p), (p, 2, 4, 700, None), (p, 0, 4, 700, p), (p, 2, 0, 700, p), (p, 2, 17, 700, p), (p, 2, 4, 0, p),
                 (p, 2, 4, 16385, p)):
        assert L.salsa_scene_rir_spectra(*args, None) == -1
    with pytest.raises(ValueError):
        sc.RirBank(np.zeros((2, 17, 8)), [0, 0], [0, 0])
    with pytest.raises(ValueError):
        sc.RirBank(np.zeros((2, 4, 16385)), [0, 0], [0, 0])
    with pytest.raises(ValueError):
        sc.EventPool([np.zeros(0)], [0])
    with pytest.raises(ValueError):
        sc.make_rir_bank('mic', [(0, 0)], 8)


# ------------------------------------------------------------------------------------------------------------------ the responses' directions
@pytest.fixture(scope='module')
def one_second_event():
    return _pool([24000], [2], seed=3)


def _oracle_features(oracle, fmt, pool, bank, rir, gain=0.8):
    scenes = sc.Scenes.from_items(48000, [[(0, rir, 9000, gain, 0)]], pool, bank)
    audio = sr.render64(scenes, pool, bank, 48000)[0].astype(np.float32)
    feat = oracle.extract_salsa(audio, audio_format=fmt, fmax_doa=9000 if fmt == 'foa' else 4000)
    nz = (feat[4:] != 0).any(axis=0)
    return feat[4:][:, nz], int(nz.sum())


@pytest.mark.parametrize('rir', [0, 1, 3])
def test_foa_responses_put_the_labels_direction_into_every_bin(oracle, one_second_event, rir):
    bank = _bank('foa', 64)
    got, n = _oracle_features(oracle, 'foa', one_second_event, bank, rir)
    x, y, z = sc._unit(bank.azimuth[rir], bank.elevation[rir])
    assert n > 10000
    dev = np.abs(got - np.array([y, z, x])[:, None]).max()
    print('FOA rir %d: %d bins, largest deviation %.3g' % (rir, n, dev))
    assert dev <= 1e-6


@pytest.mark.parametrize('rir', [0, 1, 3])
def test_mic_responses_put_the_path_differences_into_the_medians(oracle, one_second_event, rir):
    bank = _bank('mic', 64)
    got, n = _oracle_features(oracle, 'mic', one_second_event, bank, rir)
    mics = sc.MIC_RADIUS * sc._unit([m[0] for m in sc.MIC_DIRECTIONS], [m[1] for m in sc.MIC_DIRECTIONS])
    want = (mics[1:] - mics[0]) @ sc._unit(bank.azimuth[rir], bank.elevation[rir])
    med = np.median(got, axis=1)
    print('MIC rir %d: %d bins, medians off by %s' % (rir, n, np.abs(med / want - 1)))
    assert n > 3000
    assert np.all(np.abs(med - want) <= 0.02 * np.abs(want))


def test_bank_layout_and_tail():
    foa = _bank('foa', 300, rt60=0.3, drr_db=6.0, seed=2)
    assert foa.rirs.shape == (4, 4, 300) and foa.rirs.dtype == np.float32 and foa.audio_format == 'foa'
    x, y, z = sc._unit(70, -20)
    np.testing.assert_allclose(foa.rirs[0, :, 0], [1.0, y, z, x], rtol=1e-7)   # W, Y, Z, X on one tap
    tail = foa.rirs[:, :, 1:].astype(np.float64)
    np.testing.assert_allclose((tail ** 2).sum(-1), 10 ** -0.6, rtol=1e-5)     # 6 dB below the direct path of W
    long = _bank('foa', 2400, rt60=0.3).rirs[:, :, 1:].astype(np.float64)     # 0.1 s of a 0.3-s rt60: 20 dB down
    assert 50 < (long[..., :100] ** 2).sum() / (long[..., -100:] ** 2).sum() < 200
    assert np.array_equal(_bank('foa', 300, rt60=0.3, seed=2).rirs, foa.rirs)
    assert not np.array_equal(_bank('foa', 300, rt60=0.3, seed=3).rirs, foa.rirs)
    dry = _bank('foa', 300)
    assert not dry.rirs[:, :, 1:].any()
    mic = _bank('mic', 64)
    assert mic.rirs.shape == (4, 4, 64) and not mic.rirs[:, :, 33:].any()
    np.testing.assert_allclose(mic.rirs.sum(-1), 1.0, atol=2e-3)               # a fractional delay has unit gain at DC
    pool = sc.synth_event_pool(5, 2, 1)
    assert len(pool) == 10 and list(pool.classes) == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4] and pool.flat.dtype == np.float32
    again = sc.synth_event_pool(5, 2, 1)
    assert all(np.array_equal(a, b) for a, b in zip(pool.signals, again.signals))
    assert all(abs(np.abs(s).max() - 0.5) < 1e-6 for s in pool.signals)


def test_lane_arithmetic_of_the_transforms_on_the_cpu(tmp_path):
    """salsa_amd/csrc/scene_fft.h compiled with g++: the Stockham addressing, the real-transform unpack / pack and one overlap-save
    block, lane by lane as the kernels run them, against float64"""
    import subprocess
    root = os.path.dirname(_lib.INCLUDE_DIR)
    exe = str(tmp_path / 'scene_fft_emu')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-I', _lib.CSRC_DIR,
                           os.path.join(root, 'tests', 'hostemu', 'scene_fft_emu.cpp'), '-o', exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    errs = [float(line.split()[-1]) for line in r.stdout.splitlines()]
    assert len(errs) == 3 and 0 < errs[0] < 2e-5 and 0 < errs[1] < 1e-5 and 0 < errs[2] < 1e-6
