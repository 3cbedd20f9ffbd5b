"""CPU tests of the shoebox image-source responses (salsa_amd/rooms.py): the definition's analytic cases on the
float64 restatement of tests/room_reference.py, the host-side image table, the public path on the CPU (the composed torch evaluation)
against that restatement, the Eyring conversion as a formula, the refusals -- the launcher's before any device call --, the table-level
reference against the room-level one, the hand-built tables of tests/room_tables.py (what they claim; the launcher takes them) and the ABI."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import room_reference as rr
from salsa_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE, BETA, ARRAY = (3.1, 2.3, 2.7), (0.9, 0.85, 0.8, 0.75, 0.7, 0.65), (1.4, 1.1, 1.2)
DIRECTIONS = [(-60, 20), (135, -35), (0, 90)]


def _window(x):
    return np.where(np.abs(x) < rr.H, np.sinc(x) * 0.5 * (1.0 + np.cos(np.pi * x / rr.H)), 0.0)


# ---- the definition's analytic cases, on the reference -------------------------------------------------------------------------
def test_all_beta_zero_leaves_the_direct_image_with_make_rir_banks_gains():
    from salsa_amd import scenes as sc
    length, dist, direction = 64, 0.9, (-130, 40)
    src = rr.source(ARRAY, direction, dist)
    imgs = rr.images(SIZE, (0.0,) * 6, rr.d_max_of(length, src[1]))
    assert [(n, q, a, o) for n, q, a, o in imgs] == [((0, 0, 0), (0, 0, 0), 1.0, 0)]
    h, reached = rr.response(imgs, SIZE, src, rr.receivers('foa', ARRAY), True, length)
    tau = dist * rr.FS / rr.SOUND_SPEED - src[1]
    assert src[1] == math.floor(dist * rr.FS / rr.SOUND_SPEED) - rr.H and rr.H <= tau < rr.H + 1        # the peak sits near tap H
    gains = sc.make_rir_bank('foa', [direction], 1).rirs[0, :, 0].astype(np.float64)                      # (1, u_y, u_z, u_x) in float32
    want = gains[:, None] * _window(np.arange(length) - tau)[None]
    assert np.abs(h - want).max() <= 1e-7                       # the gains' float32 rounding, 6e-8; everything else is float64
    assert np.array_equal(reached[0], np.abs(np.arange(length) - tau) < rr.H) and not h[:, ~reached[0]].any()


def test_a_far_mic_source_tends_to_make_rir_banks_plane_wave():
    """At D = 1000 m, aligned and normalised, capsule m differs from the plane-wave kernel of make_rir_bank('mic') by
      * its gain D / |s - rho_m| = 1 + O(r / D), r = MIC_RADIUS: at most r / D (1 + r / D) = 4.3e-5 of a kernel whose peak is 1,
      * its delay: |s - rho_m| = D - u . m + e, 0 <= e <= r^2 / (2 D) = 8.8e-7 m = 6.2e-5 samples, and D fs / c - floor(D fs / c) = phi
        samples that all capsules share (D is chosen with phi <= 1e-6); the kernel's slope is at most 1.4 per sample,
    and the float32 rounding of make_rir_bank's array, 6e-8.  Bound: r / D (1 + r / D) + 1.4 (r^2 / (2 D) fs / c + phi) + 6e-8 = 1.3e-4.
    (The gain term is first order in r / D; MIC_RADIUS^2 / distance bounds the delay term alone.)  Measured on the reference: 8.3e-5."""
    from salsa_amd import scenes as sc
    D = (69971 + 5e-7) * rr.SOUND_SPEED / rr.FS
    phi = D * rr.FS / rr.SOUND_SPEED - 69971
    assert abs(D - 1000.0) < 0.01 and 0 <= phi <= 1e-6
    r = rr.MIC_RADIUS
    bound = r / D * (1 + r / D) + 1.4 * (r * r / (2 * D) * rr.FS / rr.SOUND_SPEED + phi) + 6e-8
    assert bound < 1.4e-4
    size, array, length = (3000.0, 3000.0, 3000.0), (1500.0, 1500.0, 1500.0), 2 * rr.H + 1
    worst = 0.0
    for direction in [(30, 10), (-100, -20), (170, 40), (0, 90)]:
        src = rr.source(array, direction, D)
        assert src[1] == 69971 - rr.H
        imgs = rr.images(size, (0.0,) * 6, rr.d_max_of(length, src[1]))
        h, _ = rr.response(imgs, size, src, rr.receivers('mic', array), False, length)
        want = sc.make_rir_bank('mic', [direction], length).rirs[0].astype(np.float64)
        worst = max(worst, float(np.abs(h - want).max()))
    print('far field: largest difference %.3g, bound %.3g' % (worst, bound))
    assert worst <= bound


def test_one_reflecting_wall_gives_two_images():
    beta = (0.5, 0.0, 0.0, 0.0, 0.0, 0.0)
    length, dist, direction = 400, 0.7, (-60, 20)
    src = rr.source(ARRAY, direction, dist, align_direct=False, normalize_direct=False)
    imgs = rr.images(SIZE, beta, rr.d_max_of(length, 0))
    assert [(n, q, a, o) for n, q, a, o in imgs] == [((0, 0, 0), (0, 0, 0), 1.0, 0), ((0, 0, 0), (1, 0, 0), 0.5, 1)]
    h, _ = rr.response(imgs, SIZE, src, rr.receivers('foa', ARRAY), True, length)
    s, a = src[0], np.asarray(ARRAY)
    want = np.zeros((4, length))
    for p, amp in ((s, 1.0), (np.array([-s[0], s[1], s[2]]), 0.5)):            # the source, and its mirror image in the wall x = 0
        d = np.linalg.norm(p - a)
        u = (p - a) / d
        want += (amp / d) * np.array([1.0, u[1], u[2], u[0]])[:, None] * _window(np.arange(length) - d * rr.FS / rr.SOUND_SPEED)[None]
    assert np.abs(h - want).max() <= 1e-14 * np.abs(want).max()
    assert np.abs(h[0]).max() > 1.0 and (h[3] < 0).any()                       # 1 / 0.7 on W; the image lies at negative x


def test_six_distinct_betas_name_their_walls():
    """the first-order image in every wall: where it lies, and whose coefficient it carries"""
    from salsa_amd import rooms
    s = np.array([0.9, 1.6, 0.5])
    first = {}
    for n, q, amp, order in rr.images(SIZE, BETA, 8.0):
        if order == 1:
            p = (1.0 - 2.0 * np.array(q)) * s + 2.0 * np.array(n) * np.array(SIZE)
            first[amp] = p
    assert sorted(first) == sorted(BETA)
    for ax in range(3):
        for side, wall in ((0, 0.0), (1, SIZE[ax])):
            want = s.copy()
            want[ax] = 2.0 * wall - s[ax]
            assert np.allclose(first[BETA[2 * ax + side]], want, atol=1e-12), (ax, side)
    tab = rooms.room_images(rooms.ShoeboxRoom(SIZE, beta=BETA, array=ARRAY), 8.0)
    one = tab.order == 1
    got = {float(a): sg * s + sh for a, sg, sh in zip(tab.amplitude[one], tab.sign[one], tab.shift[one])}
    assert sorted(got) == sorted(BETA) and all(np.allclose(got[b], first[b], atol=1e-12) for b in BETA)


def test_mirroring_room_and_source_in_y_flips_channel_y_alone():
    length = 500
    beta_m = (BETA[0], BETA[1], BETA[3], BETA[2], BETA[4], BETA[5])
    array_m = (ARRAY[0], SIZE[1] - ARRAY[1], ARRAY[2])
    for direction in DIRECTIONS[:2]:
        src = rr.source(ARRAY, direction, 0.7)
        src_m = rr.source(array_m, (-direction[0], direction[1]), 0.7)
        d_max = rr.d_max_of(length, src[1])
        h, _ = rr.response(rr.images(SIZE, BETA, d_max), SIZE, src, rr.receivers('foa', ARRAY), True, length)
        hm, _ = rr.response(rr.images(SIZE, beta_m, d_max), SIZE, src_m, rr.receivers('foa', array_m), True, length)
        assert np.abs(h[1]).max() > 0.1
        assert np.abs(hm * np.array([1.0, -1.0, 1.0, 1.0])[:, None] - h).max() <= 1e-12 * np.abs(h).max()


# ---- room_images ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('max_order', [None, 3])
def test_room_images_is_the_closed_form_in_canonical_order(max_order):
    from salsa_amd import rooms
    room = rooms.ShoeboxRoom(SIZE, beta=BETA, array=ARRAY)
    d_max = 9.0
    tab = rooms.room_images(room, d_max, max_order)
    box = rr.images(SIZE, BETA, d_max, max_order)
    key = [tuple(n) + tuple(q) for n, q in zip(tab.n.tolist(), tab.q.tolist())]
    assert key == sorted(key) and len(set(key)) == len(key) and len(key) > (20 if max_order else 200)
    by_key = {n + q: (a, o) for n, q, a, o in box}
    assert [k for k in (n + q for n, q, _, _ in box) if k in set(key)] == key, 'the relative order of the brute-force enumeration'
    assert np.array_equal(tab.order, [by_key[k][1] for k in key])
    assert np.allclose(tab.amplitude, [by_key[k][0] for k in key], rtol=1e-14, atol=0)
    assert np.array_equal(tab.sign, 1.0 - 2.0 * tab.q) and np.array_equal(tab.shift, 2.0 * tab.n * np.array(SIZE))
    assert tab.table().shape == (7, len(key)) and tab.table().dtype == np.float64
    # the cut is conservative: an image that was left out is farther than d_max from any receiver, wherever the source is
    rng = np.random.RandomState(0)
    left_out = [k for k in by_key if k not in set(key)]
    assert left_out or max_order                                               # (every image of order <= 3 lies within 9 m)
    pts = rng.uniform(0.0, 1.0, (40, 2, 3)) * np.array(SIZE)
    for k in left_out:
        p = (1.0 - 2.0 * np.array(k[3:])) * pts[:, 0] + 2.0 * np.array(k[:3]) * np.array(SIZE)
        assert np.sqrt(((p - pts[:, 1]) ** 2).sum(axis=1)).min() > d_max


def test_room_images_order_zero_and_absent_images():
    from salsa_amd import rooms
    room = rooms.ShoeboxRoom(SIZE, beta=BETA, array=ARRAY)
    tab = rooms.room_images(room, 50.0, max_order=0)
    assert len(tab) == 1 and not tab.n.any() and not tab.q.any() and tab.amplitude[0] == 1.0 and tab.order[0] == 0
    dead = rooms.room_images(rooms.ShoeboxRoom(SIZE, beta=0.0), 50.0)
    assert len(dead) == 1 and dead.order[0] == 0
    wall = rooms.room_images(rooms.ShoeboxRoom(SIZE, beta=(0.5, 0, 0, 0, 0, 0)), 50.0)
    assert wall.q.tolist() == [[0, 0, 0], [1, 0, 0]] and not wall.n.any() and wall.amplitude.tolist() == [1.0, 0.5]
    half = rooms.room_images(rooms.ShoeboxRoom(SIZE, beta=(0.9, 0.8, 0, 0.7, 0.6, 0)), 12.0)
    assert np.all(half.amplitude > 0) and len(half) > 10
    assert not np.any(np.abs(half.n[:, 1] - half.q[:, 1]) > 0) and not np.any(np.abs(half.n[:, 2]) > 0)   # no bounce off a dead wall


# ---- the public path on the CPU ------------------------------------------------------------------------------------------------
def _reference_bank(fmt, size, beta, array, directions, distance, length, max_order=None, align=True, normalize=True):
    out = []
    for direction in directions:
        src = rr.source(array, direction, distance, align, normalize)
        imgs = rr.images(size, beta, rr.d_max_of(length, src[1]), max_order)
        out.append(rr.reference_and_yardstick(imgs, size, src, rr.receivers(fmt, array), fmt == 'foa', length))
    return out


@pytest.mark.parametrize('fmt', ['foa', 'mic'])
def test_the_cpu_path_meets_the_float64_reference(fmt):
    from salsa_amd import rooms, scenes as sc
    length = 300
    room = rooms.ShoeboxRoom(SIZE, beta=BETA, array=ARRAY)
    bank = sc.room_rir_bank(fmt, room, DIRECTIONS, 0.7, length, device='cpu')
    assert isinstance(bank, sc.RirBank) and bank.rirs.shape == (3, 4, length) and bank.rirs.dtype == np.float32
    assert bank.audio_format == fmt and bank.azimuth.tolist() == [-60, 135, 0] and bank.elevation.tolist() == [20, -35, 90]
    assert not bank._spectra
    for r, (ref, Y, reached) in enumerate(_reference_bank(fmt, SIZE, BETA, ARRAY, DIRECTIONS, 0.7, length)):
        err = float(np.abs(bank.rirs[r].astype(np.float64) - ref).max())
        print('RATIO cpu %s source %d err %.3e yard %.3e ratio %.2f' % (fmt, r, err, Y, err / Y))
        assert Y > 0 and err <= rr.bound(ref, Y)
        assert np.array_equal(bank.rirs[r][~reached].view(np.uint32), np.zeros((~reached).sum(), np.uint32)), '+0.0 outside every support'
        assert abs(ref[0]).max() > 0.5
    again = sc.room_rir_bank(fmt, room, DIRECTIONS, [0.7, 0.7, 0.7], length, device='cpu')
    assert np.array_equal(again.rirs.view(np.uint32), bank.rirs.view(np.uint32))
    third = rooms.room_rir_bank(fmt, room, DIRECTIONS[2:], 0.7, length, device='cpu')
    assert np.array_equal(third.rirs[0].view(np.uint32), bank.rirs[2].view(np.uint32)), 'a source alone'


def test_the_cpu_path_options():
    """no alignment, no normalisation, an order limit and a near source, against the reference"""
    from salsa_amd import rooms
    room = rooms.ShoeboxRoom(SIZE, beta=BETA, array=ARRAY)
    for kw, ref_kw, dist in ((dict(align_direct=False), dict(align=False), 0.05), (dict(normalize_direct=False), dict(normalize=False), 0.7),
                             (dict(max_order=1), dict(max_order=1), 0.7)):
        bank = rooms.room_rir_bank('foa', room, DIRECTIONS[:1], dist, 200, device='cpu', **kw)
        ref, Y, _ = _reference_bank('foa', SIZE, BETA, ARRAY, DIRECTIONS[:1], dist, 200, **ref_kw)[0]
        assert np.abs(bank.rirs[0].astype(np.float64) - ref).max() <= rr.bound(ref, Y), kw
    zero = rooms.room_rir_bank('foa', room, DIRECTIONS[:1], 0.7, 200, max_order=0, device='cpu')
    dead = rooms.room_rir_bank('foa', rooms.ShoeboxRoom(SIZE, beta=0.0, array=ARRAY), DIRECTIONS[:1], 0.7, 200, device='cpu')
    assert np.array_equal(zero.rirs.view(np.uint32), dead.rirs.view(np.uint32)) and np.abs(zero.rirs).max() > 0.5


# ---- the Eyring conversion, as a formula ---------------------------------------------------------------------------------------
def test_rt60_is_eyrings_uniform_beta():
    from salsa_amd import rooms
    size, rt60, c = (6.0, 5.0, 3.2), 0.3, 343.0
    V, S = 6.0 * 5.0 * 3.2, 2.0 * (6.0 * 5.0 + 5.0 * 3.2 + 6.0 * 3.2)
    alpha = 1.0 - math.exp(-24.0 * math.log(10.0) * V / (c * S * rt60))
    assert abs(alpha - 0.32656) < 1e-4                                         # by hand: 24 ln 10 x 96 / (343 x 130.4 x 0.3) = 0.39537
    room = rooms.ShoeboxRoom(size, rt60=rt60)
    assert room.rt60 == rt60 and np.allclose(room.beta, math.sqrt(1.0 - alpha), rtol=1e-14, atol=0) and room.beta.shape == (6,)
    assert np.array_equal(room.array, [3.0, 2.5, 1.6])
    slow = rooms.ShoeboxRoom(size, rt60=0.6, c=340.0)
    assert np.allclose(slow.beta ** 2, math.exp(-24.0 * math.log(10.0) * V / (340.0 * S * 0.6)), rtol=1e-14, atol=0)
    assert rooms.eyring_beta(size, 1e9) > 1 - 1e-6 and rooms.eyring_beta(size, 1e-3) < 1e-20


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_python_refusals():
    from salsa_amd import rooms, scenes as sc
    room = rooms.ShoeboxRoom(SIZE, beta=BETA, array=ARRAY)
    with pytest.raises(ValueError, match='exactly one of beta and rt60'):
        rooms.ShoeboxRoom(SIZE)
    with pytest.raises(ValueError, match='exactly one of beta and rt60'):
        rooms.ShoeboxRoom(SIZE, beta=0.5, rt60=0.3)
    for bad in (dict(beta=1.5), dict(beta=(0.5,) * 5), dict(beta=0.5, array=(0.0, 1.0, 1.0)), dict(beta=0.5, array=(1.0, 2.3, 1.0))):
        with pytest.raises(ValueError):
            rooms.ShoeboxRoom(SIZE, **bad)
    with pytest.raises(ValueError, match='source lies outside the room'):
        rooms.room_rir_bank('foa', room, [(0, 0)], 1.8, 100, device='cpu')        # 1.4 + 1.8 > 3.1
    with pytest.raises(ValueError, match='source lies outside the room'):
        rooms.room_rir_bank('foa', room, [(0, 0), (0, -90)], [0.5, 1.2], 100, device='cpu')     # on the floor: not strictly inside
    with pytest.raises(ValueError, match='receiver lies outside the room'):
        rooms.room_rir_bank('mic', rooms.ShoeboxRoom(SIZE, beta=0.5, array=(0.02, 1.0, 1.0)), [(0, 0)], 0.5, 100, device='cpu')
    with pytest.raises(ValueError, match='within 0.001 m of a receiver'):
        rooms.room_rir_bank('foa', room, [(0, 0)], 0.0005, 100, device='cpu')
    with pytest.raises(ValueError, match='within 0.001 m of a receiver'):          # on capsule 0 of the tetrahedron
        rooms.room_rir_bank('mic', room, [sc.MIC_DIRECTIONS[0]], sc.MIC_RADIUS, 100, device='cpu')
    with pytest.raises(ValueError, match='length'):
        rooms.room_rir_bank('foa', room, [(0, 0)], 0.5, sc.MAX_RIR_LEN + 1, device='cpu')
    with pytest.raises(ValueError, match='length'):
        rooms.room_rir_bank('foa', room, [(0, 0)], 0.5, 0, device='cpu')
    with pytest.raises(ValueError, match='audio_format'):
        rooms.room_rir_bank('stereo', room, [(0, 0)], 0.5, 100, device='cpu')
    with pytest.raises(ValueError, match='distance'):
        rooms.room_rir_bank('foa', room, [(0, 0), (10, 0)], [0.5, 0.5, 0.5], 100, device='cpu')
    with pytest.raises(ValueError, match='too many images'):
        rooms.room_rir_bank('foa', rooms.ShoeboxRoom((1.0, 1.0, 1.0), beta=0.99), [(0, 0)], 0.2, sc.MAX_RIR_LEN, device='cpu')


def _launch(**over):
    """salsa_room_rirs on host tables that are in order, with fake device pointers: every refusal comes before a device call"""
    a = dict(images=np.array([[1.0], [1.0], [-1.0], [0.0], [0.0], [4.0], [0.5]]), n_images=1,
             sources=np.array([[1.0, 1.0, 1.0, 0.0, 1.0]]), n_sources=1, receivers=np.array([[1.5, 1.0, 1.0]]), n_receivers=1, mode=1,
             fs_over_c=70.0, rir_len=100, d_images=0x1000, d_sources=0x2000, out=0x3000)
    a.update(over)
    keep = [np.ascontiguousarray(a[k], np.float64) if a[k] is not None else None for k in ('images', 'sources', 'receivers')]
    hp = lambda x: C.c_void_p(x.ctypes.data) if x is not None else None
    return _lib.load().salsa_room_rirs(hp(keep[0]), C.c_void_p(a['d_images']), a['n_images'], hp(keep[1]), C.c_void_p(a['d_sources']),
                                       a['n_sources'], hp(keep[2]), a['n_receivers'], a['mode'], a['fs_over_c'], a['rir_len'],
                                       C.c_void_p(a['out']), None)


def test_the_launcher_refuses_before_any_device_call():
    L = _lib.load()
    assert L.salsa_room_max_images() == 1 << 22 and L.salsa_room_tap_block() == 256
    def bad_image(row, v):
        t = np.array([[1.0], [1.0], [-1.0], [0.0], [0.0], [4.0], [0.5]])
        t[row, 0] = v
        return t

    cases = [dict(images=None), dict(sources=None), dict(receivers=None), dict(d_images=0), dict(d_sources=0), dict(out=0),
             dict(n_images=0), dict(n_images=(1 << 22) + 1), dict(n_sources=0), dict(n_sources=65536), dict(n_receivers=0),
             dict(n_receivers=5), dict(n_receivers=2, receivers=np.ones((2, 3))), dict(mode=2), dict(mode=-1), dict(rir_len=0),
             dict(rir_len=16385), dict(fs_over_c=0.0), dict(fs_over_c=float('nan')), dict(fs_over_c=float('inf')),
             dict(images=bad_image(0, 0.5)), dict(images=bad_image(2, float('nan'))), dict(images=bad_image(4, float('inf'))),
             dict(images=bad_image(6, 0.0)), dict(images=bad_image(6, 1.5)), dict(images=bad_image(6, float('nan'))),
             dict(sources=np.array([[float('nan'), 1, 1, 0, 1]])), dict(sources=np.array([[1.0, 1, 1, -1, 1]])),
             dict(sources=np.array([[1.0, 1, 1, 0.5, 1]])), dict(sources=np.array([[1.0, 1, 1, 0, 0]])),
             dict(sources=np.array([[1.0, 1, 1, 0, float('inf')]])), dict(receivers=np.array([[float('nan'), 1.0, 1.0]]))]
    for over in cases:
        assert _launch(**over) == _lib.E_INVAL, over
        assert 'salsa_room_rirs' in _lib.last_error()
    assert _launch(n_receivers=2, receivers=np.ones((2, 3)), mode=1) == _lib.E_INVAL and 'FOA' in _lib.last_error()


# ---- the table-level reference and the built tables of tests/room_tables.py ----------------------------------------------------
@pytest.mark.parametrize('fmt', ['foa', 'mic'])
def test_response_of_table_gives_the_bits_of_response_on_a_rooms_table(fmt):
    from salsa_amd import rooms
    length = 300
    room = rooms.ShoeboxRoom(SIZE, beta=BETA, array=ARRAY)
    _, sources, receivers, d_max = rooms.room_geometry(fmt, room, DIRECTIONS[:1], 0.7, length)
    tab = rooms.room_images(room, d_max)
    image_list = list(zip(map(tuple, tab.n.tolist()), map(tuple, tab.q.tolist()), tab.amplitude.tolist(), tab.order.tolist()))
    assert len(image_list) > 100
    src = rr.source(ARRAY, DIRECTIONS[0], 0.7)
    assert np.array_equal(src[0], sources[0, :3]) and src[1] == sources[0, 3] and src[2] == sources[0, 4]
    recs = rr.receivers(fmt, ARRAY)
    for kw in (dict(), dict(f32=True), dict(f32=True, reverse=True), dict(reverse=True)):
        h, reached = rr.response(image_list, SIZE, src, recs, fmt == 'foa', length, **kw)
        ht, reached_t = rr.response_of_table(tab.table(), src, recs, fmt == 'foa', length, rr.FS / rr.SOUND_SPEED, **kw)
        assert h.dtype == ht.dtype == (np.float32 if kw.get('f32') else np.float64) and np.abs(h).max() > 0.5
        assert np.array_equal(h.view(np.uint8), ht.view(np.uint8)) and np.array_equal(reached, reached_t), kw
    fwd = rr.response_of_table(tab.table(), src, recs, fmt == 'foa', length, rr.FS / rr.SOUND_SPEED, f32=True)[0]
    rev = rr.response_of_table(tab.table(), src, recs, fmt == 'foa', length, rr.FS / rr.SOUND_SPEED, f32=True, reverse=True)[0]
    assert not np.array_equal(fwd, rev), 'the order of the float32 sum shows'


def _accepted(table, src_row, mode=1, fs_over_c=None, rir_len=None):
    """the launcher's host checks pass the table and the source: its LAST check, the receivers', is the one that refuses (no device call)"""
    import room_tables as rt
    rc = _launch(images=table, n_images=table.shape[1], sources=src_row, mode=mode, fs_over_c=fs_over_c or rt.FS_OVER_C,
                 rir_len=rir_len or rt.LENGTH, receivers=np.array([[float('nan'), 1.0, 1.0]]))
    return rc == _lib.E_INVAL and 'a receiver position is not finite' in _lib.last_error()


def _tau(table, t0=0.0):
    """the delays of a built table at the point it was built around"""
    import room_tables as rt
    p = table[0:3] * rt.SOURCE[:, None] + table[3:6]
    return np.sqrt(((p - rt.RECEIVER[:, None]) ** 2).sum(axis=0)) * rt.FS_OVER_C - t0


def test_the_built_tables_are_what_they_claim_and_the_launcher_takes_them():
    import room_tables as rt
    H, src = rr.H, rt.source()
    for name, mask in rt.MASKS.items():
        table = rt.built_table(mask)
        assert table.shape == (7, len(mask)) and table.dtype == np.float64 and _accepted(table, rt.source_row(src)), name
        tf = np.floor(_tau(table))
        kept = (tf >= -H) & (tf <= 256 + H - 2)                                 # what block 0 of the kernel keeps, by its header
        assert np.array_equal(kept, mask) and np.all(tf[mask] >= 20) and np.all(tf[~mask] > 1e7), name
        assert np.all((table[6] > 0.05) & (table[6] <= 1.0))
        full = rt.built_table(np.ones(len(mask), bool))
        assert np.array_equal(table[:, mask], full[:, mask]), 'an image does not depend on the mask'
    waves = rt.MASKS['waves_0_2'].reshape(4, 4, 64).sum(axis=2)
    assert np.array_equal(waves, [[64, 0, 64, 0]] * 4) and rt.MASKS['chunk1_miss'].reshape(4, 256).sum(axis=1).tolist() == [256, 0, 256, 256]
    assert np.nonzero(rt.MASKS['last_only'])[0].tolist() == [1023] and not rt.MASKS['none'].any()
    assert (np.floor(_tau(rt.built_table(rt.MASKS['all_1024']))) >= 256 - H).sum() > 50, 'block 1 keeps images too'
    # negative delays: t0 > 0, every floor(tau) in [-16, 3]
    neg, nsrc = rt.negative_delay_table(), rt.source(t0=40.0)
    assert _accepted(neg, rt.source_row(nsrc))
    tau = _tau(neg, 40.0)
    assert neg.shape[1] > 256 and tau.min() > -16.0 and tau.max() < 4.0 and (tau < 0).sum() > 200
    # the exact tables, and the two closed forms of the order check by a sequential float32 sum
    big = rt.big_first_table()
    assert big.shape == (7, 4097) and _accepted(big, rt.source_row(rt.exact_source(rt.BIG_TAP)), fs_over_c=1.0)
    assert rt.sequential_float32(big, float(rt.BIG_TAP), rt.LENGTH)[0, rt.BIG_TAP] == np.float32(1.0)
    assert rt.sequential_float32(big[:, ::-1], float(rt.BIG_TAP), rt.LENGTH)[0, rt.BIG_TAP] == np.float32(1.0 + 2.0 ** -13)
    table, d = rt.random_exact_table()
    assert table.shape == (7, 1000) and _accepted(table, rt.source_row(rt.exact_source(29.0)), fs_over_c=1.0)
    assert sorted(set(d.tolist())) == [29, 33, 45, 261, 290] and np.bincount(d)[[29, 33, 45, 261, 290]].min() > 100
    seq, rev = rt.sequential_float32(table, 29.0, rt.LENGTH), rt.sequential_float32(table[:, ::-1], 29.0, rt.LENGTH)
    assert (seq != 0).any(axis=1).all() and (seq < 0).any() and not np.array_equal(seq, rev), 'every channel is used, and the order shows'
    # a control: the same call with a table that is out of order is refused by the table's check, not the receivers'
    bad = table.copy()
    bad[6, 999] = 0.0
    assert not _accepted(bad, rt.source_row(rt.exact_source(29.0)), fs_over_c=1.0) and 'amplitude' in _lib.last_error()


# ---- ABI -----------------------------------------------------------------------------------------------------------------------
NEW_EXPORTS = ('salsa_room_rirs', 'salsa_room_max_images', 'salsa_room_tap_block')


def test_the_new_entry_points_are_declared_bound_and_exported():
    from salsa_amd import rooms, scenes as sc
    header = open(os.path.join(ROOT, 'include', 'salsa_hip.h')).read()
    L = _lib.load()
    for name in NEW_EXPORTS:
        assert name + '(' in header and name in _lib.EXPORTS and hasattr(L, name)
    assert _lib.PROTOTYPES['salsa_hip.h']['salsa_room_rirs'][1] == [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                                    C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p]
    assert os.path.join(_lib.CSRC_DIR, 'room_rir.hip') in _lib.build_command()
    assert open(os.path.join(_lib.CSRC_DIR, 'room_rir.hip')).read().split('\n#include')[1].strip() == '"build_guard.h"'
    assert rooms.MAX_IMAGES == L.salsa_room_max_images() and rooms.TAP_BLOCK == L.salsa_room_tap_block()
    for name in ('ShoeboxRoom', 'room_images', 'room_rir_bank'):                 # scenes re-exports the module's public names
        assert getattr(sc, name) is getattr(rooms, name)
    with pytest.raises(AttributeError):
        sc.no_such_name
