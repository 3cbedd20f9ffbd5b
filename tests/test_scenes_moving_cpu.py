"""Moving sources in the scene renderer without a GPU: the windows, the float64 restatement against a direct
time-varying sum, rows and labels of moving items against the CSV readers, the seeded draw, the segment tables, the new launcher's
refusals (decided before any device call) and the directions a moving item's audio carries, read back by the CPU oracle."""
import ctypes as C
import io

import numpy as np
import pytest

import scene_moving_reference as mr
import scene_reference as sr
from salsa_amd import _lib
from salsa_amd import scenes as sc
from salsa_amd.dataset import load_classwise_gt, load_trackwise_gt
from salsa_amd.synth import _ar1

HOP = 2400
STEPS = (240, 512, 700, 2400)


def _pool(lengths, classes, seed=1):
    rng = np.random.RandomState(seed)
    return sc.EventPool([(0.1 * _ar1(rng.randn(n + 8))[8:]).astype(np.float32) for n in lengths], classes)


def _ring(n=36, elevation=20, length=64, **kw):
    return sc.make_rir_bank('foa', [((360 // n) * j - 180, elevation) for j in range(n)], length, **kw)


def _traj(length, S, first, n_rirs, stride=1):
    return [(first + stride * k) % n_rirs for k in range(int(sc.traj_nodes(length, S)))]


# ------------------------------------------------------------------------------------------------------------------ windows
@pytest.mark.parametrize('S', STEPS)
def test_windows_sum_to_one_and_node_counts_follow_the_formula(S):
    for ln in (1, 2, S, S + 1, 2 * S, 2 * S + 1, 3000):
        K = int(sc.traj_nodes(ln, S))
        assert K == -(-(ln - 1) // S) + 1 == mr.n_nodes(ln, S) and (K == 1) == (ln == 1)
        total = sum(mr.window64(k, S, ln) for k in range(K))
        assert np.abs(total - 1.0).max() <= 2.0 ** -52, (S, ln)
        assert mr.window64(K, S, ln).max() <= 0.0                              # a node more would weigh nothing: K nodes suffice
        for k in range(K):                                                     # node k's window lives on ((k - 1) S, (k + 1) S) only
            w = mr.window64(k, S, ln)
            nz = np.nonzero(w)[0]
            assert len(nz) and nz[0] == max(0, (k - 1) * S + 1) and nz[-1] == min(ln, (k + 1) * S) - 1
    with pytest.raises(ValueError):
        sc.Scenes.from_items(4000, [[(0, [0, 1], 0, 1.0, 0)]], _pool([3000], [0]), _ring(), traj_step=S)    # K is not 2 for 3000 samples


# ------------------------------------------------------------------------------------------------------------------ the float64 restatement
def _small_scene(S=240):
    pool = _pool([700, 1500, 1], [0, 1, 2])
    bank = sc.make_rir_bank('foa', [(10 * j - 40, 5 * j) for j in range(9)], 60, rt60=0.2, seed=4)
    items = [(0, _traj(700, S, 0, 9), 17, 0.9, 0), (1, 2, 900, 0.4, 1), (1, _traj(1500, S, 8, 9, 2), 2200, 1.1, 0), (2, [5], 3000, 0.7, 1)]
    return sc.Scenes.from_items(4133, [items], pool, bank, traj_step=S), pool, bank


def test_render64_moving_is_the_direct_time_varying_sum():
    scenes, pool, bank = _small_scene()
    S = scenes.traj_step
    amb = (0.01 * np.random.RandomState(5).randn(1, 4, 4133)).astype(np.float32)
    ref = mr.render64_moving(scenes, pool, bank, 4133, amb)
    assert ref.dtype == np.float64
    for c, n in ((0, 17), (2, 300), (1, 760), (3, 1000), (0, 2500), (2, 3000), (3, 4132), (1, 16)):
        want = float(amb[0, c, n])
        for i in range(scenes.n_items):
            e, o, g = int(scenes.event[i]), int(scenes.onset[i]), float(scenes.gain[i])
            s = pool.signals[e].astype(np.float64)
            nodes = scenes.traj_rir[scenes.nodes(i)] if scenes.traj_start[i + 1] > scenes.traj_start[i] else None
            for m in range(len(s)):
                if not 0 <= n - o - m < bank.length:
                    continue
                if nodes is None:
                    want += g * s[m] * float(bank.rirs[scenes.rir[i], c, n - o - m])
                else:
                    want += g * s[m] * sum(max(0.0, 1.0 - abs(m - k * S) / S) * float(bank.rirs[r, c, n - o - m]) for k, r in enumerate(nodes))
        assert abs(ref[0, c, n] - want) < 1e-12, (c, n)
    m = mr.support(scenes, pool, bank, 4133)
    assert m[0, 17] and not m[0, 16] and np.array_equal(ref[0][:, ~m[0]], amb[0][:, ~m[0]].astype(np.float64))
    top, errs = mr.float32_yardstick(scenes, pool, bank, 4133, amb, ref)
    assert len(errs) == 4 and all(0 < e < 1e-5 * np.abs(ref).max() for e in errs)


@pytest.mark.parametrize('S', STEPS)
def test_a_constant_trajectory_is_the_static_item(S):
    pool = _pool([700, 3000, 1, 2], [0, 1, 2, 3])
    bank = sc.make_rir_bank('foa', [(10, 0), (-60, 20), (120, -30)], 300, rt60=0.2, seed=2)
    rows = [(0, 1, 17, 0.9, 0), (1, 2, 500, 0.4, 1), (2, 0, 5, 1.0, 2), (3, 1, 4131, 1.0, 2), (1, 0, 3000, 0.5, 0)]
    static = sc.Scenes.from_items(4133, [rows], pool, bank)
    moving = sc.Scenes.from_items(4133, [[(e, [r] * int(sc.traj_nodes(pool.lengths[e], S)), o, g, t) for e, r, o, g, t in rows]], pool, bank,
                                  traj_step=S)
    assert moving.has_trajectories and not static.has_trajectories
    ref = sr.render64(static, pool, bank, 4133)
    assert np.abs(mr.render64_moving(moving, pool, bank, 4133) - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.array_equal(mr.render64_moving(static, pool, bank, 4133), ref)   # no trajectory: the old definition itself
    assert np.array_equal(sc.scene_rows(moving[0]), sc.scene_rows(static[0]))


# ------------------------------------------------------------------------------------------------------------------ rows and labels
def _label_scene(S):
    """20 label frames.  Item 0: an onset that is no multiple of 2400; item 1: onset 5 * 2400 + 1200 - S, so that node 1 sits exactly
    on the centre of frame 5; then two moving items of class 5 on two tracks, a one-sample item (K = 1), and an item cut by the
    clip's end."""
    pool = _pool([3 * HOP + 100, 2 * HOP, 4000, 1, 3 * HOP, 2 * HOP + 5], [0, 1, 7, 2, 5, 5])
    bank = _ring()
    L = [int(n) for n in pool.lengths]
    items = [(0, _traj(L[0], S, 0, 36), 1337, 1.0, 0),
             (1, _traj(L[1], S, 5, 36, 2), 5 * HOP + HOP // 2 - S, 0.5, 1),
             (4, _traj(L[4], S, 20, 36), 9 * HOP + 17, 1.0, 0),
             (5, _traj(L[5], S, 30, 36, 35), 10 * HOP, 0.7, 1),
             (3, [7], 17 * HOP + 5, 1.0, 0),
             (2, _traj(L[2], S, 11, 36), 48000 - 1000, 1.0, 1)]
    return sc.Scenes.from_items(48000, [items], pool, bank, traj_step=S), pool, bank


@pytest.mark.parametrize('S', [240, 700, 2400])
def test_rows_carry_the_node_nearest_the_frame_centre(S):
    scenes, pool, bank = _label_scene(S)
    rows = sc.scene_rows(scenes[0])
    assert scenes.onset[0] % HOP != 0 and int(sc.traj_nodes(1, S)) == 1
    seen_change = False
    for i in range(scenes.n_items):
        o, ln = int(scenes.onset[i]), int(scenes.length[i])
        nodes = scenes.traj_rir[scenes.nodes(i)]
        K = len(nodes)
        mine = rows[(rows[:, 1] == scenes.cls[i]) & (rows[:, 2] == scenes.track[i])]
        frames = list(range(o // HOP, (min(o + ln, 48000) - 1) // HOP + 1))     # active where the dry extent meets the frame, as before
        assert list(mine[:, 0]) == frames
        for f, az, el in mine[:, [0, 3, 4]]:
            centre = HOP * f + HOP // 2 - o                                    # the frame's centre in the item's dry time
            k = mr.frame_node(f, o, S, K)
            d = np.abs(np.arange(K) * S - centre)
            assert d[k] == d.min() and (k == K - 1 or d[k + 1] > d[k])        # the nearest node; of two equally near, the later
            assert (az, el) == (bank.azimuth[nodes[k]], bank.elevation[nodes[k]])
        seen_change = seen_change or len(set(mine[:, 3])) > 1
        assert scenes.azimuth[i] == bank.azimuth[nodes[0]] and scenes.rir[i] == nodes[0]
    assert seen_change
    # a node time exactly on a frame centre: node 1 of item 1 on the centre of frame 5
    o = int(scenes.onset[1])
    assert HOP * 5 + HOP // 2 - o == S
    row = rows[(rows[:, 0] == 5) & (rows[:, 1] == 1)][0]
    assert row[3] == bank.azimuth[scenes.traj_rir[scenes.nodes(1)][1]] != bank.azimuth[scenes.traj_rir[scenes.nodes(1)][0]]
    # a frame centre midway between two nodes: the later node is taken.  Onset 1200 - S / 2 puts the centre of frame 0 there.
    assert S % 2 == 0
    tie = sc.Scenes.from_items(48000, [[(1, _traj(2 * HOP, S, 5, 36, 2), HOP // 2 - S // 2, 1.0, 0)]], pool, bank, traj_step=S)
    assert 2 * (HOP // 2 - int(tie.onset[0])) == S
    assert sc.scene_rows(tie[0])[0].tolist() == [0, 1, 0, bank.azimuth[7], 20] and tie.azimuth[0] == bank.azimuth[5]


@pytest.mark.parametrize('fmt', ['classwise', 'trackwise'])
@pytest.mark.parametrize('S', [240, 2400])
def test_labels_of_moving_items_equal_the_csv_readers_bit_for_bit(tmp_path, fmt, S):
    scenes, pool, bank = _label_scene(S)
    drawn = sc.draw_scenes(2, sc.synth_event_pool(12, 2, 3), bank, 8 * 24000, 11, max_polyphony=3, allow_same_class=True, moving=1.0,
                           speed_deg_s=(60.0, 120.0), traj_step=S)
    for k, scene in enumerate([scenes[0], drawn[0], drawn[1]]):
        n_lab = scene.n_samples // HOP
        fn = str(tmp_path / ('meta%d.csv' % k))
        rows = sc.scene_rows(scene)
        np.savetxt(fn, rows, fmt='%d', delimiter=',')
        want = load_classwise_gt(fn, 8 * n_lab, 12) if fmt == 'classwise' else load_trackwise_gt(fn, 8 * n_lab, 12)[:2]
        got = sc.scene_labels(scene, n_lab, 12, fmt)
        for g, w in zip(got, want):
            assert g.dtype == np.float32 and g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32))
        assert got[0].sum() > 0
        per_item = [rows[(rows[:, 1] == c) & (rows[:, 2] == t)] for c, t in set(map(tuple, rows[:, 1:3]))]
        assert any(len(set(map(tuple, r[:, 3:]))) > 1 for r in per_item)       # some direction changes from frame to frame
    sed, doa = sc.scene_labels(scenes[0], 20, 12, fmt)
    if fmt == 'trackwise':                                                     # both moving items of class 5 are kept, in two slots
        assert sed[11, 5] == 1 and sed[11, 12 + 5] == 1 and sed[9, 12 + 5] == 0
    else:
        assert sed[11, 5] == 1
    assert sed[19, 7] == 1 and sed[17, 2] == 1


# ------------------------------------------------------------------------------------------------------------------ draws
def _angle(az0, el0, az1, el1):
    return np.degrees(np.arccos(np.clip(np.sum(sc._unit(az0, el0) * sc._unit(az1, el1), axis=-1), -1.0, 1.0)))


def test_nearest_takes_the_least_angle_and_the_lowest_index():
    bank = sc.make_rir_bank('foa', [(0, 0), (90, 0), (0, 0), (180, 0), (-90, 60)], 8)
    assert bank.nearest(10, 0) == 0 and bank.nearest(44, 0) == 0 and bank.nearest(46, 0) == 1 and bank.nearest(0, 0) == 0
    assert bank.nearest(-179, 5) == 3 and bank.nearest(179, -5) == 3 and bank.nearest(-90, 80) == 4 and bank.nearest(123, 89) == 4
    assert list(bank.nearest(np.array([10.0, 100.0, -170.0]), np.array([0.0, 0.0, 0.0]))) == [0, 1, 3]


def test_draw_without_moving_is_the_old_draw_and_with_moving_is_seeded():
    pool = sc.synth_event_pool(6, 3, 7)
    bank = sc.make_rir_bank('foa', [(a, e) for a in range(-180, 180, 10) for e in (-20, 20)], 16)
    N = 30 * 24000
    old, zero = sc.draw_scenes(3, pool, bank, N, 5), sc.draw_scenes(3, pool, bank, N, 5, moving=0.0)
    for f in sc.Scenes.FIELDS + ('clip_start',):
        assert np.array_equal(getattr(old, f), getattr(zero, f)), f
    for s in (old, zero):
        assert not s.has_trajectories and len(s.traj_rir) == 0 and not s.traj_start.any() and len(s.traj_start) == s.n_items + 1
    for S, speed in ((2400, (10.0, 40.0)), (700, (30.0, 90.0))):
        a = sc.draw_scenes(3, pool, bank, N, 5, moving=1.0, speed_deg_s=speed, traj_step=S)
        b = sc.draw_scenes(3, pool, bank, N, 5, moving=1.0, speed_deg_s=speed, traj_step=S)
        for f in sc.Scenes.FIELDS + sc.Scenes.TRAJ_FIELDS + ('clip_start', 'traj_start'):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
        assert a.traj_step == S and a.n_items > 12 and np.array_equal(np.diff(a.traj_start), sc.traj_nodes(a.length, S))
        assert np.array_equal(a.traj_azimuth, bank.azimuth[a.traj_rir]) and np.array_equal(a.rir, a.traj_rir[a.traj_start[:-1]])
        assert np.all(a.traj_elevation == np.repeat(a.elevation, np.diff(a.traj_start)))              # it moves in azimuth only
        spacing = 10.0                                                         # no point of a ring lies further than half of it from a response
        moved = 0
        for i in range(a.n_items):
            az, el = a.traj_azimuth[a.nodes(i)], a.traj_elevation[a.nodes(i)]
            step = _angle(az[:-1], el[:-1], az[1:], el[1:])
            assert np.all(step <= speed[1] * S / sc.FS + spacing + 1e-9)
            d = (np.diff(az) + 180) % 360 - 180                                # one sense of rotation throughout
            assert np.all(d >= 0) or np.all(d <= 0)
            moved += len(set(az)) > 1
        assert moved > a.n_items // 2
        sub = a.clips(1, 3)
        assert sub.n_clips == 2 and sub.traj_start[0] == 0 and sub.traj_start[-1] == len(sub.traj_rir) and sub.traj_step == S
        assert np.array_equal(sub.traj_rir, a.traj_rir[a.traj_start[a.clip_start[1]]:])
        assert np.array_equal(sc.scene_rows(a[2]), sc.scene_rows(sub[1]))
    some = sc.draw_scenes(3, pool, bank, N, 5, moving=0.5)
    n = np.diff(some.traj_start)
    assert (n == 0).any() and (n > 0).any()


# ------------------------------------------------------------------------------------------------------------------ segment tables
def _brute_block_table(clip_start, segs, N, L):
    M, P = -(-N // 512), -(-L // 512)
    tab = np.zeros((len(clip_start) - 1, M, 2), np.int32)
    for b in range(len(clip_start) - 1):
        for m in range(M):
            reach = [s for s in range(clip_start[b], clip_start[b + 1])
                     if segs[1, s] // 512 <= m <= min(min((segs[1, s] + segs[2, s] - 1) // 512 + 1, M - 1) + P - 1, M - 1)]
            tab[b, m] = (reach[0], reach[-1] + 1) if reach else (clip_start[b], clip_start[b])
    return tab


@pytest.mark.parametrize('S', STEPS)
def test_segment_tables_cover_every_item(S):
    scenes, pool, bank = _small_scene(S)
    two = sc.Scenes.from_items(4133, [[], [(1, _traj(1500, S, 0, 9), 3000, 1.0, 0), (0, 3, 4132, 1.0, 1)]], pool, bank, traj_step=S)
    for sce in (scenes, two):
        clip_start, segs, gains, block, longest = sc.segment_tables(sce, pool, bank)
        assert segs.dtype == np.int64 and segs.shape[0] == 6 and gains.dtype == np.float32 and block.dtype == np.int32
        assert clip_start[0] == 0 and clip_start[-1] == segs.shape[1] == len(gains) and longest == segs[2].max() <= max(2 * S - 1, 1500)
        want = [seg for b in range(sce.n_clips) for seg in mr.expand(sce, pool, b, 4133)]               # the independent restatement
        assert segs.shape[1] == len(want)
        for s, (e, a, end, r, centre, o, g) in enumerate(want):
            assert tuple(segs[:4, s]) == (pool.offset[e] + a, o + a, end - a, r) and gains[s] == g
            assert tuple(segs[4:, s]) == ((0, 0) if centre is None else (centre - a, S))
        q_max = segs[2] - 1
        windowed = segs[5] != 0
        assert np.all(np.abs(segs[4][windowed]) < S) and np.all(np.abs(q_max - segs[4])[windowed] < S)   # |q - centre| < step at both ends
        s = 0
        for b in range(sce.n_clips):
            for i in range(sce.clip_start[b], sce.clip_start[b + 1]):
                ln, K = int(sce.length[i]), int(sce.traj_start[i + 1] - sce.traj_start[i])
                covered = np.zeros(ln, int)                                    # how many of the item's segments hold each dry sample
                for _ in range(max(K, 1)):
                    a = segs[1, s] - sce.onset[i] if s < clip_start[b + 1] else -1
                    if 0 <= a < ln and a == segs[0, s] - pool.offset[sce.event[i]]:
                        covered[a:a + segs[2, s]] += 1
                        assert (segs[5, s] == 0) == (K == 0)
                        s += 1
                in_clip = np.arange(ln) + sce.onset[i] < 4133                  # only segments that start past the clip's end are left out
                assert np.all(covered[in_clip] >= 1) and covered.max() <= 2 and (K or np.all(covered == 1))
        assert s == segs.shape[1]
        # the block table leaves out no reaching segment, stays inside its clip, and is empty or tight where segments do not nest
        exact = _brute_block_table(clip_start, segs, 4133, bank.length)
        some = exact[..., 1] > exact[..., 0]
        assert np.all(block[..., 0][some] <= exact[..., 0][some]) and np.all(block[..., 1][some] >= exact[..., 1][some])
        assert np.all(block[..., 0] <= block[..., 1])
        for b in range(sce.n_clips):
            assert block[b].min() >= clip_start[b] and block[b].max() <= clip_start[b + 1]
        if sce is two:
            assert np.array_equal(block, exact)
    static = sc.Scenes.from_items(4133, [[(1, 2, 900, 0.4, 1), (0, 0, 4000, 1.0, 0)]], pool, bank)
    clip_start, segs, gains, block, longest = sc.segment_tables(static, pool, bank)
    assert segs.T.tolist() == [[700, 900, 1500, 2, 0, 0], [0, 4000, 700, 0, 0, 0]] and longest == 1500


# ------------------------------------------------------------------------------------------------------------------ ABI
NEW_EXPORTS = ('salsa_scene_render_moving', 'salsa_scene_moving_workspace_bytes')
N_ABI, L_ABI = 4133, 700


def test_exports_and_size_query():
    L = _lib.load()
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert _lib.PROTOTYPES['salsa_hip.h']['salsa_scene_moving_workspace_bytes'] == (C.c_size_t, [C.c_int64, C.c_int, C.c_int])
    assert L.salsa_abi_version() == 2
    # segments x min((max_segment_len + 510) / 512 + 2, ceil(N / 512)) x 4096
    assert L.salsa_scene_moving_workspace_bytes(1440000, 1, 1) == 2 * 4096
    assert L.salsa_scene_moving_workspace_bytes(1440000, 479, 7) == 7 * 3 * 4096
    assert L.salsa_scene_moving_workspace_bytes(1440000, 4799, 8192) == 8192 * 12 * 4096     # S = 2400: 12 slots whatever the event's length
    assert L.salsa_scene_moving_workspace_bytes(1440000, 72000, 960) == L.salsa_scene_workspace_bytes(1440000, 72000, 960)
    assert L.salsa_scene_moving_workspace_bytes(4133, 100000, 5) == 5 * 9 * 4096
    assert L.salsa_scene_moving_workspace_bytes(4133, 3000, 0) == 0
    for bad in ((0, 100, 1), (4133, 0, 1), (4133, 100, -1)):
        assert L.salsa_scene_moving_workspace_bytes(*bad) == 0


def _moving_args(**over):
    """a call that would be valid -- with HOST pointers everywhere, so that a launch with it would be an error"""
    segs = np.array([[0, 100, 240, 0, 0, 240], [1, 101, 479, 1, 239, 240], [100, 3000, 1000, 1, 0, 0]], np.int64).T.copy()
    clip_start = np.array([0, 2, 3], np.int32)
    a = dict(events=np.zeros(5000, np.float32), n_event_samples=5000, spectra=np.zeros(4096, np.float32), R=2, Cn=4, L=L_ABI,
             clip_start=clip_start, segs=segs, gains=np.ones(3, np.float32), block=_brute_block_table(clip_start, segs, N_ABI, L_ABI),
             n_clips=2, n_segs=3, max_len=1000, ambient=np.zeros(8, np.float32), out=np.zeros(8, np.float32), N=N_ABI,
             ws=np.zeros(8, np.float32), ws_bytes=1 << 30)
    a.update(over)
    return a


def _moving(a):
    p = lambda x: None if x is None else C.c_void_p(x.ctypes.data)
    return _lib.load().salsa_scene_render_moving(p(a['events']), a['n_event_samples'], p(a['spectra']), a['R'], a['Cn'], a['L'],
                                                 p(a['clip_start']), p(a['segs']), p(a['gains']), p(a['block']), p(a['segs']), p(a['gains']),
                                                 p(a['block']), a['n_clips'], a['n_segs'], a['max_len'], p(a['ambient']), p(a['out']),
                                                 a['N'], p(a['ws']), a['ws_bytes'], None)


def _segs_with(row, col, value):
    segs = _moving_args()['segs'].copy()
    segs[row, col] = value
    return segs


def _block_with(b, m, which, value):
    block = _moving_args()['block'].copy()
    block[b, m, which] = value
    return block


BAD_MOVING = {
    'no events': dict(events=None), 'no spectra': dict(spectra=None), 'no clip_start': dict(clip_start=None), 'no segments': dict(segs=None),
    'no gains': dict(gains=None), 'no out': dict(out=None), 'no workspace': dict(ws=None), 'no block table': dict(block=None),
    'no channel': dict(Cn=0), '17 channels': dict(Cn=17), 'no response': dict(R=0), 'rir length 0': dict(L=0), 'rir too long': dict(L=16385),
    'no clip': dict(n_clips=0), 'negative segments': dict(n_segs=-1), 'no sample': dict(N=0), 'segment length 0': dict(max_len=0),
    'clip_start not from 0': dict(clip_start=np.array([1, 2, 3], np.int32)), 'clip_start not to n_segs': dict(clip_start=np.array([0, 2, 2], np.int32)),
    'clip_start decreasing': dict(clip_start=np.array([0, 4, 3], np.int32)),
    'onset at N': dict(segs=_segs_with(1, 2, 4133)), 'onset negative': dict(segs=_segs_with(1, 0, -1)),
    'length 0': dict(segs=_segs_with(2, 2, 0)), 'length above the maximum': dict(segs=_segs_with(2, 2, 1001)),
    'samples past the pool': dict(segs=_segs_with(0, 2, 4001)), 'samples before the pool': dict(segs=_segs_with(0, 0, -1)),
    'rir index': dict(segs=_segs_with(3, 2, 2)), 'rir negative': dict(segs=_segs_with(3, 0, -1)),
    'gain not finite': dict(gains=np.array([1, np.inf, 1], np.float32)), 'gain nan': dict(gains=np.array([np.nan, 1, 1], np.float32)),
    'step below 240': dict(segs=_segs_with(5, 0, 239)), 'step negative': dict(segs=_segs_with(5, 0, -240)),
    'step above 2^24': dict(segs=_segs_with(5, 2, (1 << 24) + 1)),
    'ramp zero at the first sample': dict(segs=_segs_with(4, 1, 240)), 'ramp zero before the first sample': dict(segs=_segs_with(4, 1, -240)),
    'ramp zero at the last sample': dict(segs=_segs_with(4, 1, 238)), 'ramp below zero at the end': dict(segs=_segs_with(2, 0, 300)),
    'a window on a long static segment': dict(segs=_segs_with(5, 2, 240)),
    'block table leaves out the last reaching segment': dict(block=_block_with(0, 0, 1, 1)),
    'block table leaves out the first reaching segment': dict(block=_block_with(0, 1, 0, 1)),
    'block table empty where a segment reaches': dict(block=_block_with(1, 7, 1, 2)),
    'block range before its clip': dict(block=_block_with(1, 0, 0, 1)), 'block range past its clip': dict(block=_block_with(0, 8, 1, 3)),
    'block range reversed': dict(block=_block_with(0, 8, 0, 1)),
}


def test_the_valid_call_of_the_refusal_table_is_refused_only_for_its_workspace():
    """the table above changes ONE thing each in a call that passes every host check: shown by its reaching the workspace check"""
    need = _lib.load().salsa_scene_moving_workspace_bytes(N_ABI, 1000, 3)
    assert need == 3 * 4 * 4096
    assert _moving(_moving_args(ws_bytes=need - 1)) == -5 and 'workspace' in _lib.last_error()
    block = _moving_args()['block']
    assert block[0, 0].tolist() == [0, 2] and block[0, 8].tolist() == [0, 0] and block[1, 7].tolist() == [2, 3] and block[1, 0].tolist() == [2, 2]


@pytest.mark.parametrize('what', sorted(BAD_MOVING))
def test_moving_render_refuses_before_any_device_call(what):
    assert _moving(_moving_args(ws_bytes=0, **BAD_MOVING[what])) == -1, what    # -1 and not -5: refused before the workspace is looked at
    assert 'salsa_scene_render_moving' in _lib.last_error()


def test_moving_render_refuses_more_than_its_stated_segments_per_clip():
    many = sc.MAX_SEGMENTS_PER_CLIP + 1
    segs = np.tile(np.array([[0], [0], [1], [0], [0], [0]], np.int64), (1, many))
    clip_start = np.array([0, many, many], np.int32)
    block = np.zeros((2, 9, 2), np.int32)                                     # a one-sample segment at onset 0 reaches blocks 0, 1 and 2
    block[0, :3, 1] = many
    block[0, 3:], block[1] = many, many
    a = _moving_args(clip_start=clip_start, segs=segs, gains=np.ones(many, np.float32), n_segs=many, block=block, ws_bytes=0)
    assert _moving(a) == -1 and '65536' in _lib.last_error()
    ok = many - 1                                                              # 65536 in one clip pass every table check
    block[0, :3, 1], block[0, 3:], block[1] = ok, ok, ok
    a = _moving_args(clip_start=np.array([0, ok, ok], np.int32), segs=segs[:, :ok].copy(), gains=np.ones(ok, np.float32), n_segs=ok,
                     block=block, ws_bytes=0)
    assert _moving(a) == -5
    with pytest.raises(ValueError):
        sc.Scenes(4133, [0, 1], event=[0], rir=[0], onset=[0], gain=[1.0], cls=[0], track=[0], length=[500], azimuth=[0], elevation=[0],
                  traj_start=[0, 4], traj_rir=[0, 0, 0, 0], traj_azimuth=[0] * 4, traj_elevation=[0] * 4, traj_step=239)


# ------------------------------------------------------------------------------------------------------------------ the oracle reads the motion back
@pytest.mark.parametrize('onset', [9000, 9137])
def test_the_oracle_reads_each_nodes_direction_at_its_time(oracle, onset):
    """anechoic FOA ring of 36 azimuths at elevation 20, a 1-s AR(1) event moving one bank step per node (S = 2400): in the STFT frame
    nearest each node time the median angle, over the non-zero bins, between the feature's direction and the node's label is at most a
    quarter of the node spacing at interior nodes and half of it at the two end nodes."""
    S, hop = 2400, 300
    bank = _ring(36, 20, 64)
    pool = sc.EventPool([(0.1 * _ar1(np.random.RandomState(3).randn(24000))).astype(np.float32)], [2])
    K = int(sc.traj_nodes(24000, S))
    traj = [(3 + k) % 36 for k in range(K)]
    scenes = sc.Scenes.from_items(48000, [[(0, traj, onset, 0.8, 0)]], pool, bank, traj_step=S)
    audio = mr.render64_moving(scenes, pool, bank, 48000)[0].astype(np.float32)
    feat = oracle.extract_salsa(audio, audio_format='foa', fmax_doa=9000)
    spacing = float(_angle(bank.azimuth[3], 20, bank.azimuth[4], 20))
    assert K == 11 and abs(spacing - 9.4) < 0.05
    medians, worst = [], 0.0
    for k in range(K):
        t = int(round((onset + k * S) / hop))
        v = feat[4:, t, :]
        nz = (v != 0).any(axis=0)
        assert nz.sum() > 50
        x, y, z = sc._unit(bank.azimuth[traj[k]], bank.elevation[traj[k]])
        cosine = (np.array([y, z, x]) @ v[:, nz]) / np.linalg.norm(v[:, nz], axis=0)
        ang = np.degrees(np.arccos(np.clip(cosine, -1.0, 1.0)))
        medians.append(float(np.median(ang)))
        worst = max(worst, float(ang.max()))
    print('onset %d: spacing %.2f, interior medians %.2f - %.2f, end-node medians %.2f %.2f, worst single bin %.2f'
          % (onset, spacing, min(medians[1:-1]), max(medians[1:-1]), medians[0], medians[-1], worst))
    assert max(medians[1:-1]) <= spacing / 4 and max(medians[0], medians[-1]) <= spacing / 2
