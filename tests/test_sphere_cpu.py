"""CPU tests of the rigid-sphere capsule model (salsa_amd/rooms.py: baffle='rigid') against the float64 restatement
of tests/sphere_reference.py: the series, the table against the series, the low-frequency phase ratio, the composed torch path, the
unchanged defaults and the refusals (those of salsa_room_rirs_sphere included: each comes before any device call).

The three errors of the table are MEASURED here, relative to the table's peak (1.497), on a grid the table does not contain (60 of the
odd quarter-degrees, random fractions), and asserted at twice the measured value rounded up to one digit -- the margin covers a later
change of grid:
    support truncation     2.02e-3  ->  TRUNCATION_BOUND = 5e-3     (the whole band-limited sum against the one cut to [-16, 32))
    angle interpolation    5.55e-4  ->  ANGLE_BOUND      = 2e-3     (fractions on the phase grid)
    phase interpolation    3.12e-4  ->  PHASE_BOUND      = 7e-4     (angles on the angle grid)
Low-frequency ratio: the least-squares ratio of the rigid to the open inter-capsule phases over 90 - 400 Hz (six capsule pairs) is
1.5176 .. 1.5246 over the 30 x 40 degree grid of directions: a deviation of LF_MEASURED = 0.025 from 1.5 (the sphere's next-order
term at k R = 0.07 .. 0.31); LF_BOUND is twice that."""
import ctypes as C
import functools

import numpy as np
import pytest

import sphere_reference as sr

TRUNCATION_BOUND, ANGLE_BOUND, PHASE_BOUND = 5e-3, 2e-3, 7e-4
LF_MEASURED = 0.025
LF_BOUND = 2 * LF_MEASURED
SIZE, BETA, DISTANCE = (3.0, 4.0, 2.5), 0.7, 0.7
ARRAY = (1.5, 2.0, 1.25)
DIRECTIONS = ((45, 35), (-60, 20), (170, -50))                                  # the first on capsule 0's axis: Theta = 0 and the three other angles
LENGTHS = (300, 513)


@functools.lru_cache(maxsize=None)
def ref_table():
    S = sr.table()
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def off_grid():
    """(theta (60,): odd quarter-degrees, their sphere filters) -- shared, never written"""
    rng = np.random.RandomState(1)
    deg = np.arange(0.25, 180, 0.5)
    theta = np.deg2rad(deg[rng.permutation(len(deg))[:60]])
    return theta, sr.sphere_filter(theta)


TAPS = np.arange(-sr.LEAD + 1, sr.TRAIL + 1)


# ---- the series ----------------------------------------------------------------------------------------------------------------------
def test_series():
    from salsa_amd import rooms
    ct = np.cos(np.deg2rad(np.arange(0, 181, 7.5)))[None]
    assert np.all(rooms.sphere_response(0.0, ct) == 1.0)
    f = np.linspace(0, 12000, 241)[:, None]
    got, ref = rooms.sphere_response(f, ct), sr.series(f, ct)
    assert got.dtype == np.complex128 and np.abs(got - ref).max() <= 1e-12
    assert np.abs(sr.series(f, ct, order=60) - ref).max() <= 1e-13             # N = 48 truncates below float64 noise up to k R = 9.3
    # the phase slope at k R <= 0.1: 1.5 k R cos Theta, an ADVANCE at Theta = 0
    fl = np.array([20.0, 60.0, 120.0])[:, None]
    kR = 2 * np.pi * fl / rooms.SOUND_SPEED * rooms.MIC_RADIUS
    assert kR.max() <= 0.1
    assert np.all(np.abs(np.angle(rooms.sphere_response(fl, ct)) - 1.5 * kR * ct) <= kR ** 3)     # the next term of the expansion is O((k R)^3)
    # |H| at Theta = 0 grows towards 2 over 1 - 11 kHz: monotonically from kHz to kHz (1.27, 1.53, 1.71, ... 1.94, 1.95); between
    # them the series itself ripples by up to 0.008 (1.943 at 9.5 kHz, 1.935 at 10 kHz -- the reference's series gives the same), so
    # a finer grid is held to that ripple
    mag = np.abs(rooms.sphere_response(np.arange(1000.0, 11001.0, 1000.0), 1.0))
    assert np.all(np.diff(mag) > 0) and 1.9 < mag[-1] < 2.0 and mag[0] > 1.0
    fine = np.abs(rooms.sphere_response(np.arange(1000.0, 11001.0, 250.0), 1.0))
    assert np.all(np.diff(fine) > -0.01) and np.all(fine < 2.0)
    for bad in (dict(f=-1.0, cos_theta=0.0), dict(f=1.0, cos_theta=1.5)):
        with pytest.raises(ValueError):
            rooms.sphere_response(**bad)


# ---- the table -----------------------------------------------------------------------------------------------------------------------
def test_table_is_the_definition():
    from salsa_amd import rooms, scenes as sc
    st = rooms.sphere_table()
    assert st is sc.sphere_table(sr.MIC_RADIUS, sr.FS, sr.SOUND_SPEED) and isinstance(st, sc.SphereTable)
    assert (st.Q, st.P, st.lead, st.trail) == (sr.Q, sr.P, sr.LEAD, sr.TRAIL)
    assert st.table.dtype == np.float32 and st.table.shape == (sr.Q + 1, sr.P + 1, sr.LT) and not st.table.flags.writeable
    S = ref_table()
    assert np.abs(st.table.astype(np.float64) - S).max() <= sr.ulp32(np.abs(S).max())
    assert np.array_equal(st.table[:, sr.P, 1:], st.table[:, 0, :-1]) and not st.table[:, sr.P, 0].any()   # row P is row 0 one tap on
    # weights(): the float64 evaluation of the interpolated definition, at exact clamps and anywhere
    rng = np.random.RandomState(2)
    for theta, fr in [(0.0, 0.0), (np.pi, 0.0), (np.pi, float(np.nextafter(1.0, 0.0))), (0.3, 0.5)] + [(rng.rand() * np.pi, rng.rand()) for _ in range(6)]:
        assert np.abs(st.weights(theta, TAPS - fr) - sr.interp(st.table, theta, fr)).max() <= 1e-13
    assert np.abs(st.weights(np.pi, TAPS.astype(np.float64)) - st.table[sr.Q, 0]).max() <= 1e-12       # Theta = pi: row Q alone
    assert not st.weights(1.0, np.array([-sr.LEAD - 0.5, sr.TRAIL + 0.01, 1e6])).any()


def test_table_against_the_series_off_its_grid():
    """the three measured errors (the module docstring), each relative to the table's peak"""
    S = ref_table()
    peak = float(np.abs(S).max())
    theta, a = off_grid()
    rng = np.random.RandomState(3)
    truncation = angle = phase = 0.0
    for fr in list(rng.rand(6)) + [0.0]:
        truncation = max(truncation, float(np.abs(sr.h_full(theta, TAPS - fr, a) - sr.h_cut(theta, TAPS - fr, a)).max()))
    for p in (0, 5, 17):                                                        # fractions ON the phase grid: the angle alone
        cut = sr.h_cut(theta, TAPS - p / sr.P, a)
        angle = max(angle, float(np.abs(np.stack([sr.interp(S, th, p / sr.P) for th in theta]) - cut).max()))
    on = np.deg2rad(np.array([0.0, 13.0, 45.0, 90.0, 131.0, 180.0]))            # angles ON the angle grid: the phase alone
    a_on = sr.sphere_filter(on)
    for fr in rng.rand(8):
        cut = sr.h_cut(on, TAPS - fr, a_on)
        phase = max(phase, float(np.abs(np.stack([sr.interp(S, th, fr) for th in on]) - cut).max()))
    print('MEASURED truncation %.3e angle %.3e phase %.3e of the peak %.4f' % (truncation / peak, angle / peak, phase / peak, peak))
    assert truncation / peak <= TRUNCATION_BOUND and angle / peak <= ANGLE_BOUND and phase / peak <= PHASE_BOUND
    # the direct peak: early at the capsule facing the wave, late (the creeping wave) at the shadowed one
    x = np.linspace(-10, 12, 2201)
    from salsa_amd import rooms
    st = rooms.sphere_table()
    assert abs(x[np.argmax(np.abs(st.weights(0.0, x)))] + 3.0) <= 0.1 and abs(x[np.argmax(np.abs(st.weights(np.pi, x)))] - 4.8) <= 0.1


# ---- the low-frequency ratio -------------------------------------------------------------------------------------------------------
def test_low_frequency_phase_is_one_and_a_half_times_the_open_arrays():
    from salsa_amd import scenes as sc
    directions = [(az, el) for az in range(0, 360, 30) for el in range(-80, 81, 40)]
    n_fft = 4096
    f = np.arange(n_fft // 2 + 1) * (sr.FS / n_fft)
    band = (f >= 90) & (f <= 400)
    phases = []
    for baffle in ('open', 'rigid'):
        h = sc.make_rir_bank('mic', directions, 128, baffle=baffle).rirs.astype(np.float64)
        spec = np.fft.rfft(h, n_fft, axis=-1)[..., band]
        phases.append(np.stack([np.angle(spec[:, m] * np.conj(spec[:, n])) for m in range(4) for n in range(m)], axis=1))     # (R, 6, F)
    ratio = (phases[1] * phases[0]).sum(axis=(1, 2)) / (phases[0] ** 2).sum(axis=(1, 2))
    print('MEASURED rigid / open phase ratio: %.4f .. %.4f' % (ratio.min(), ratio.max()))
    assert np.abs(ratio - 1.5).max() <= LF_BOUND


# ---- the torch path ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def room_reference(r):
    """source r of the room at the longest length -> (ref64 (4, 513), [yardstick in table order, reversed], reached); a shorter
    response is its prefix"""
    src = sr.source(ARRAY, DIRECTIONS[r], DISTANCE)
    images = sr.room_image_table(SIZE, (BETA,) * 6, sr.d_max_of(max(LENGTHS), src[1]))
    args = (images, src, ARRAY, sr.capsule_units(), ref_table(), sr.LEAD, sr.TRAIL, max(LENGTHS), sr.FS / sr.SOUND_SPEED)
    ref, reached = sr.response_of_table(*args)
    yards = [sr.response_of_table(*args, f32=True, reverse=rev)[0] for rev in (False, True)]
    for a in [ref, reached] + yards:
        a.setflags(write=False)
    return ref, yards, reached


def holds(what, got, length):
    """got (3, 4, length) against the shared reference within the project's bound -> the largest error / Y"""
    worst = 0.0
    for r in range(len(DIRECTIONS)):
        ref, yards, reached = room_reference(r)
        ref, reached = ref[:, :length], reached[:, :length]
        err = float(np.abs(got[r].astype(np.float64) - ref).max())
        Y = max(float(np.abs(y[:, :length].astype(np.float64) - ref).max()) for y in yards)
        print('RATIO %s len %d source %d: err %.3e Y %.3e bound %.3e' % (what, length, r, err, Y, sr.bound(ref, Y)))
        assert np.isfinite(got[r]).all() and err <= sr.bound(ref, Y)
        assert not got[r][~reached].view(np.uint32).any(), 'a tap outside every support is +0.0'
        worst = max(worst, err / Y)
    return worst


@pytest.mark.parametrize('length', LENGTHS)
def test_torch_path_against_float64(length):
    from salsa_amd import rooms
    room = rooms.ShoeboxRoom(SIZE, beta=BETA)
    assert np.array_equal(room.array, ARRAY)
    h, directions = rooms.room_rirs('mic', room, DIRECTIONS, DISTANCE, length, device='cpu', baffle='rigid')
    assert h.shape == (3, 4, length) and directions.tolist() == [list(d) for d in DIRECTIONS]
    holds('torch cpu', h.numpy(), length)
    peak = np.abs(h.numpy()[0]).argmax(axis=-1)                                 # the direct path: the facing capsule early, the others later
    assert sr.LEAD - 4 <= peak[0] <= sr.LEAD - 2 and np.all(peak[1:] > peak[0]) and np.abs(h.numpy()[0, 0]).max() > 1.0
    open_h, _ = rooms.room_rirs('mic', room, DIRECTIONS, DISTANCE, length, device='cpu')
    assert not np.allclose(open_h.numpy()[:, :, :64], h.numpy()[:, :, :64], atol=0.05)


# ---- unchanged defaults --------------------------------------------------------------------------------------------------------------
def test_open_is_the_default_and_changes_nothing():
    from salsa_amd import rooms, scenes as sc
    room = rooms.ShoeboxRoom(SIZE, beta=BETA)
    for fmt in ('mic', 'foa'):
        a, _ = rooms.room_rirs(fmt, room, DIRECTIONS, DISTANCE, 300, device='cpu')
        b, _ = rooms.room_rirs(fmt, room, DIRECTIONS, DISTANCE, 300, device='cpu', baffle='open')
        assert np.array_equal(a.numpy().view(np.uint32), b.numpy().view(np.uint32))
        g0, g1 = rooms.room_geometry(fmt, room, DIRECTIONS, DISTANCE, 300), rooms.room_geometry(fmt, room, DIRECTIONS, DISTANCE, 300, baffle='open')
        assert all(np.array_equal(x, y) for x, y in zip(g0, g1))
        for kw in (dict(), dict(rt60=0.2, seed=3)):
            a, b = sc.make_rir_bank(fmt, DIRECTIONS, 400, **kw), sc.make_rir_bank(fmt, DIRECTIONS, 400, baffle='open', **kw)
            assert np.array_equal(a.rirs.view(np.uint32), b.rirs.view(np.uint32))
    kw = dict(length=2400, directions=((0, 0), (90, 20)), device='cpu')
    assert np.array_equal(rooms.calibrate_room(SIZE, 0.1, **kw).beta, rooms.calibrate_room(SIZE, 0.1, baffle='open', **kw).beta)


def test_make_rir_bank_rigid():
    from salsa_amd import rooms, scenes as sc
    st = rooms.sphere_table()
    bank = sc.make_rir_bank('mic', DIRECTIONS, 400, rt60=0.2, seed=3, baffle='rigid')
    dry = sc.make_rir_bank('mic', DIRECTIONS, 400, baffle='rigid')
    t0 = st.lead + st.trail
    assert bank.rirs.shape == (3, 4, 400) and bank.audio_format == 'mic' and not dry.rirs[:, :, t0 + 1:].any()
    units = sr.capsule_units()
    for r, d in enumerate(DIRECTIONS):
        for m in range(4):
            theta = float(np.arccos(np.clip(sr.unit(*d) @ units[m], -1, 1)))
            want = np.concatenate([[0.0], sr.interp(st.table, theta, 0.0)])      # taps 1 .. lead + trail: the centre at tap lead
            assert np.array_equal(dry.rirs[r, m, :t0 + 1], want.astype(np.float32))
    assert np.array_equal(bank.rirs[:, :, :t0 + 1], dry.rirs[:, :, :t0 + 1]) and np.abs(bank.rirs[:, :, t0 + 1:]).min() > 0
    with pytest.raises(ValueError):
        sc.make_rir_bank('mic', DIRECTIONS, t0, baffle='rigid')


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_host_layer():
    from salsa_amd import rooms, scenes as sc
    room = rooms.ShoeboxRoom(SIZE, beta=BETA)
    for call in (lambda **kw: rooms.room_rirs('foa', room, DIRECTIONS, DISTANCE, 300, device='cpu', **kw),
                 lambda **kw: rooms.room_rir_bank('foa', room, DIRECTIONS, DISTANCE, 300, device='cpu', **kw),
                 lambda **kw: rooms.room_geometry('foa', room, DIRECTIONS, DISTANCE, 300, **kw),
                 lambda **kw: rooms.calibrate_room(SIZE, 0.2, device='cpu', **kw),
                 lambda **kw: sc.make_rir_bank('foa', DIRECTIONS, 400, **kw)):
        with pytest.raises(ValueError, match='rigid'):
            call(baffle='rigid')
        with pytest.raises(ValueError, match='baffle'):
            call(baffle='sphere')
    with pytest.raises(ValueError, match='baffle'):
        rooms.room_rirs('mic', room, DIRECTIONS, DISTANCE, 300, device='cpu', baffle='Rigid')
    with pytest.raises(ValueError, match='plane-wave'):
        rooms.room_rirs('mic', room, DIRECTIONS, 0.3, 300, device='cpu', baffle='rigid')
    rooms.room_rirs('mic', room, DIRECTIONS, 0.3, 300, device='cpu')           # the open array takes it
    rooms.room_geometry('mic', room, DIRECTIONS, 0.43, 300, baffle='rigid')     # just past 10 R = 0.42 m


def _launch(**over):
    """salsa_room_rirs_sphere on host tables that are in order, with fake device pointers: every refusal comes before a device call"""
    from salsa_amd import _lib
    Q, P, lead, trail = over.pop('Q', 4), over.pop('P', 2), over.pop('lead', 3), over.pop('trail', 5)
    a = dict(images=np.array([[1.0], [1.0], [-1.0], [0.0], [0.0], [4.0], [0.5]]), d_images=0x1000, n_images=1,
             sources=np.array([[1.0, 1.0, 1.0, 0.0, 1.0]]), d_sources=0x2000, n_sources=1, centre=np.array([1.5, 1.0, 1.0]),
             units=np.ascontiguousarray(sr.capsule_units()), d_table=0x4000,
             table=np.ones(max(Q + 1, 1) * max(P + 1, 1) * max(lead + trail, 1), np.float32),
             fs_over_c=70.0, rir_len=100, out=0x3000)
    a.update(over)
    hp = lambda v: None if v is None else C.c_void_p(v) if isinstance(v, int) else C.c_void_p(np.ascontiguousarray(v).ctypes.data)
    keep = [None if a[k] is None or isinstance(a[k], int) else np.ascontiguousarray(a[k]) for k in ('images', 'sources', 'centre', 'units', 'table')]
    ptr = lambda v: None if v is None else C.c_void_p(v.ctypes.data)
    return _lib.load().salsa_room_rirs_sphere(ptr(keep[0]), hp(a['d_images']), a['n_images'], ptr(keep[1]), hp(a['d_sources']), a['n_sources'],
                                              ptr(keep[2]), ptr(keep[3]), ptr(keep[4]), hp(a['d_table']), Q, P, lead, trail, a['fs_over_c'],
                                              a['rir_len'], hp(a['out']), None)


def test_refusals_of_the_entry_point():
    from salsa_amd import _lib
    L = _lib.load()
    mq, mp, ms = C.c_int(), C.c_int(), C.c_int()
    assert L.salsa_room_sphere_limits(C.byref(mq), C.byref(mp), C.byref(ms)) == 1 << 27 and L.salsa_room_sphere_limits(None, None, None) == 1 << 27
    assert (mq.value, mp.value, ms.value) == (4096, 1024, 512)
    nan_table, inf_table = np.ones(5 * 3 * 8, np.float32), np.ones(5 * 3 * 8, np.float32)
    nan_table[-1], inf_table[7] = np.nan, np.inf
    bad_units = np.ascontiguousarray(sr.capsule_units())
    bad_units[2] *= 1.01
    cases = [dict(images=None), dict(d_images=None), dict(sources=None), dict(d_sources=None), dict(centre=None), dict(units=None),
             dict(table=None), dict(d_table=None), dict(out=None),
             dict(Q=0), dict(P=0), dict(Q=-3), dict(Q=mq.value + 1), dict(P=mp.value + 1), dict(lead=0), dict(trail=0),
             dict(lead=200, trail=ms.value - 199, table=np.ones(8, np.float32)), dict(lead=ms.value + 1, trail=1, table=np.ones(8, np.float32)),
             dict(table=nan_table), dict(table=inf_table), dict(units=bad_units), dict(centre=np.array([np.nan, 0.0, 0.0])),
             dict(n_images=0), dict(n_sources=0), dict(rir_len=0), dict(rir_len=16385), dict(fs_over_c=0.0), dict(fs_over_c=float('nan')),
             dict(images=np.array([[1.0], [1.0], [0.5], [0.0], [0.0], [4.0], [0.5]])), dict(images=np.array([[1.0], [1.0], [-1.0], [0.0], [0.0], [4.0], [0.0]])),
             dict(sources=np.array([[1.0, 1.0, 1.0, 0.5, 1.0]])), dict(sources=np.array([[1.0, 1.0, 1.0, 0.0, 0.0]]))]
    for over in cases:
        assert _launch(**over) == _lib.E_INVAL, over
        assert 'salsa_room_rirs_sphere' in _lib.last_error(), over
    proto = _lib.PROTOTYPES['salsa_hip.h']['salsa_room_rirs_sphere']
    assert proto[1] == [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                        C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p]
    import os
    assert os.path.join(_lib.CSRC_DIR, 'room_sphere.hip') in _lib.build_command()
