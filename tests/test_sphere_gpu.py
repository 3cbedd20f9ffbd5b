"""GPU tests of the rigid-sphere capsule kernel (salsa_amd/csrc/room_sphere.hip: salsa_room_rirs_sphere) against the
float64 restatement of tests/sphere_reference.py.  Bound of every comparison, per source: max |got - ref64| <= 4 Y + ulp32(max |ref64|)
(tests/room_reference.py: bound), Y the larger error of the float32 yardstick summed in table order and in reversed table order.

The hand-built case: fs / c = 1, the centre at the origin, source 0 at the origin with t0 = 0 and g = 1, so image i of source 0 lies AT its
shift and its delay IS its distance; the capsule units are +x, +y, +z, -x, so an image on the x axis has Theta exactly 0 and pi.  The
sphere table is random float32 of an odd shape (Q = 5, P = 3, lead = 7, trail = 9): the kernel only reads it.  600 images at 20 .. 230
samples all reach the first tap block (three compaction chunks, the last partial); the named images after them are the edges.

Measured on one MI355X, error / Y: the kernel 0.80 - 0.97 on the hand-built tables (every length alike from 255 taps on) and 0.36 - 1.00
on the real room (3 x 4 x 2.5 m, beta 0.7; errors 2.9e-8 .. 1.5e-7 against bounds of 2.8e-7 .. 7.3e-7); the torch legs 1.00."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import sphere_reference as sr
from salsa_amd import _lib
from test_sphere_cpu import ARRAY, BETA, DIRECTIONS, DISTANCE, LENGTHS, SIZE, holds

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARD = 67                                                                     # floats on either side of the output: odd, so `out` is 4-byte aligned only
BLOCK = 256
HQ, HP, HLEAD, HTRAIL = 5, 3, 7, 9
UNITS = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0]])
CENTRE = np.zeros(3)
SOURCES = np.array([[0.0, 0.0, 0.0, 0.0, 1.0], [0.5, 0.25, 0.0, 0.0, 1.0], [-1.0, 2.0, 0.5, 3.0, 0.7]])      # position, t0, g
HAND_LENGTHS = (1, 255, 256, 257, 300)


@functools.lru_cache(maxsize=None)
def hand_table():
    S = np.random.RandomState(11).uniform(-1.0, 1.0, (HQ + 1, HP + 1, HLEAD + HTRAIL)).astype(np.float32)
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def hand_images():
    """(7, 600 + edges): the dense chunk, then the named edges on the x axis (Theta = 0 for capsule 0, pi for capsule 3, or the reverse)"""
    rng = np.random.RandomState(12)
    u = rng.randn(600, 3)
    u /= np.sqrt((u * u).sum(axis=1, keepdims=True))
    pos = list(u * rng.uniform(20.0, 230.0, 600)[:, None])
    edges = [40.0,                                   # an exactly integer delay: fraction 0
             float(np.nextafter(1.0, 0.0)),          # the largest float64 fraction below 1 (floor tau = 0: the support cut at tap 0)
             float(np.nextafter(41.0, 0.0)),         # the largest fraction an image at tap 40 can have
             -50.0,                                  # Theta = pi for capsule 0, 0 for capsule 3
             2.3,                                    # a support cut at tap 0
             BLOCK - HTRAIL + 0.5, BLOCK - HTRAIL - 0.5,               # last tap = tap 256, the first of block 1 / tap 255: misses block 1
             BLOCK + HLEAD - 2 + 0.25, BLOCK + HLEAD - 1 + 0.25,       # first tap = tap 255, the last of block 0 / tap 256: misses block 0
             300 + HLEAD - 2 + 0.75, 300 + HLEAD - 1.0,                # first tap = tap 299 / tap 300: the end of the longest response
             254.0 + HLEAD - 1, 255.0 + HLEAD - 1]                     # first tap = tap 254 and 255, the cuts of lengths 255 and 256
    pos += [np.array([x, 0.0, 0.0]) for x in edges]
    pos = np.array(pos)
    n = len(pos)
    table = np.concatenate([np.ones((3, n)), pos.T, rng.uniform(0.2, 1.0, (1, n))])
    table.setflags(write=False)
    return table


@functools.lru_cache(maxsize=None)
def hand_reference(r):
    """source r at the longest length -> (ref64, [yardsticks], reached); a shorter response is its prefix"""
    src = (SOURCES[r, :3], SOURCES[r, 3], SOURCES[r, 4])
    args = (hand_images(), src, CENTRE, UNITS, hand_table(), HLEAD, HTRAIL, max(HAND_LENGTHS), 1.0)
    ref, reached = sr.response_of_table(*args)
    yards = [sr.response_of_table(*args, f32=True, reverse=rev)[0] for rev in (False, True)]
    for a in [ref, reached] + yards:
        a.setflags(write=False)
    return ref, yards, reached


def run(images, sources, centre, units, S, lead, trail, fs_over_c, length):
    """salsa_room_rirs_sphere, the output inside NaN guard bands -> numpy (R, 4, length)"""
    images, sources = np.array(images, np.float64, order='C'), np.array(sources, np.float64, order='C')      # (copies: the shared tables are read-only)
    centre, units, S = np.array(centre, np.float64, order='C'), np.array(units, np.float64, order='C'), np.array(S, np.float32, order='C')
    R, n = len(sources), len(sources) * 4 * length
    buf = torch.full((n + 2 * GUARD,), float('nan'), dtype=torch.float32, device=DEV)
    d_images, d_sources, d_S = torch.from_numpy(images).to(DEV), torch.from_numpy(sources).to(DEV), torch.from_numpy(S).to(DEV)
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc = _lib.load().salsa_room_rirs_sphere(p(images), C.c_void_p(d_images.data_ptr()), images.shape[1], p(sources), C.c_void_p(d_sources.data_ptr()), R,
                                            p(centre), p(units), p(S), C.c_void_p(d_S.data_ptr()), S.shape[0] - 1, S.shape[1] - 1, lead, trail,
                                            fs_over_c, length, C.c_void_p(buf[GUARD:].data_ptr()),
                                            C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all()), 'a guard band was written'
    out = buf[GUARD:GUARD + n].view(R, 4, length)
    assert not bool(torch.isnan(out).any()), 'an output element was not written'
    return out.cpu().numpy()


def run_hand(length, n_sources=3, units=UNITS):
    return run(hand_images(), SOURCES[:n_sources], CENTRE, units, hand_table(), HLEAD, HTRAIL, 1.0, length)


def hand_holds(got, length):
    for r in range(got.shape[0]):
        ref, yards, reached = hand_reference(r)
        ref, reached = ref[:, :length], reached[:, :length]
        err = float(np.abs(got[r].astype(np.float64) - ref).max())
        Y = max(float(np.abs(y[:, :length].astype(np.float64) - ref).max()) for y in yards)
        print('RATIO hand len %d source %d: err %.3e Y %.3e bound %.3e' % (length, r, err, Y, sr.bound(ref, Y)))
        assert np.isfinite(got[r]).all() and err <= sr.bound(ref, Y)
        assert not got[r][~reached].view(np.uint32).any(), 'a tap outside every support is +0.0'


# ---- hand-built tables through the C entry point ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_sources', [1, 3])
@pytest.mark.parametrize('length', HAND_LENGTHS)
def test_kernel_against_float64_on_hand_built_tables(length, n_sources):
    got = run_hand(length, n_sources)
    hand_holds(got, length)
    assert np.abs(got).max() > 0.01


def test_the_named_edges_are_what_they_claim():
    """the reference's own view of the edge images of source 0: exact fractions, exact angles, and supports that end where the docstring says"""
    import math
    tab = hand_images()
    d = tab[3, 600:]
    assert d[0] == 40.0 and d[1] - math.floor(d[1]) == 1.0 - 2.0 ** -53 and math.floor(d[2]) == 40
    for x, (q0, w0, q3, w3) in ((40.0, (0, 0.0, HQ - 1, 1.0)), (-50.0, (HQ - 1, 1.0, 0, 0.0))):
        c = x / abs(x)
        for cos, q, wq in ((c, q0, w0), (-c, q3, w3)):                          # Theta = pi: the rows Q - 1 and Q, weights (0, 1) to float32
            got = sr.cell(math.acos(cos), 0.0, HQ, HP)
            assert got[0] == q and np.float32(got[1]) == np.float32(wq)
    assert sr.cell(0.0, d[1], HQ, HP)[2] == HP - 1                              # the largest fraction reads the phases P - 1 and P
    k0 = np.floor(d).astype(int)
    first, last = k0 - HLEAD + 1, k0 + HTRAIL
    assert last[5] == BLOCK and last[6] == BLOCK - 1 and first[7] == BLOCK - 1 and first[8] == BLOCK
    assert first[9] == 299 and first[10] == 300 and first[11] == 254 and first[12] == 255 and first[4] < 0


def test_a_block_no_image_reaches_is_plus_zero():
    length = 3 * BLOCK - 40
    rng = np.random.RandomState(13)
    x = np.concatenate([rng.uniform(5.0, 150.0, 40), [BLOCK - HTRAIL - 1 + 0.5, 2 * BLOCK + HLEAD - 1 + 0.5], rng.uniform(600.0, 700.0, 40)])
    images = np.concatenate([np.ones((3, len(x))), [x, 0 * x, 0 * x], rng.uniform(0.2, 1.0, (1, len(x)))])
    got = run(images, SOURCES[:1], CENTRE, UNITS, hand_table(), HLEAD, HTRAIL, 1.0, length)
    ref, Y, reached = sr.table_reference(images, (SOURCES[0, :3], 0.0, 1.0), CENTRE, UNITS, hand_table(), HLEAD, HTRAIL, length, 1.0)
    assert np.abs(got[0].astype(np.float64) - ref).max() <= sr.bound(ref, Y)
    assert not reached[:, BLOCK:2 * BLOCK].any() and reached[:, BLOCK - 1].all() and reached[:, 2 * BLOCK].all()
    assert not got[0][~reached].view(np.uint32).any() and np.abs(got[0][:, :BLOCK]).max() > 0.01 and np.abs(got[0][:, 2 * BLOCK:]).max() > 1e-3   # (A / d: 1 / 650 there)


# ---- exact properties ------------------------------------------------------------------------------------------------------------------
def test_exact_properties():
    length = 300
    batch = run_hand(length)
    assert np.array_equal(run_hand(length).view(np.uint32), batch.view(np.uint32)), 'two runs give equal bits'
    for r in range(3):
        alone = run(hand_images(), SOURCES[r:r + 1], CENTRE, UNITS, hand_table(), HLEAD, HTRAIL, 1.0, length)
        assert np.array_equal(alone[0].view(np.uint32), batch[r].view(np.uint32)), 'a source alone gives the bits it has in a batch'
    for m in range(4):                                                          # capsule m's row does not depend on the other capsules' directions
        other = np.roll(UNITS, 1, axis=0) * np.array([1.0, -1.0, 1.0])
        other[m] = UNITS[m]
        moved = run_hand(length, units=other)
        assert np.array_equal(moved[:, m].view(np.uint32), batch[:, m].view(np.uint32))
        assert not np.array_equal(moved, batch)


# ---- a real room -----------------------------------------------------------------------------------------------------------------------
def _public_tables(length):
    from salsa_amd import rooms
    room = rooms.ShoeboxRoom(SIZE, beta=BETA)
    _, sources, _, d_max = rooms.room_geometry('mic', room, DIRECTIONS, DISTANCE, length, baffle='rigid')
    return room, rooms.room_images(room, d_max).table(), sources, rooms.sphere_table()


@pytest.mark.parametrize('length', LENGTHS)
def test_a_real_room_against_float64(length, monkeypatch):
    from salsa_amd import rooms
    room = rooms.ShoeboxRoom(SIZE, beta=BETA)
    h, _ = rooms.room_rirs('mic', room, DIRECTIONS, DISTANCE, length, device=DEV, baffle='rigid')
    holds('HIP', h.cpu().numpy(), length)
    monkeypatch.setattr(rooms, 'HIP_ROOM', False)                               # SALSA_HIP_ROOM=0: the composed torch leg on the device
    leg, _ = rooms.room_rirs('mic', room, DIRECTIONS, DISTANCE, length, device=DEV, baffle='rigid')
    holds('torch on the device', leg.cpu().numpy(), length)


def test_the_public_path_runs_the_kernel_and_the_switch_leaves_it(monkeypatch):
    from salsa_amd import rooms, scenes as sc
    room, images, sources, st = _public_tables(300)
    direct = run(images, sources, room.array, sr.capsule_units(), st.table, st.lead, st.trail, sr.FS / sr.SOUND_SPEED, 300)
    bank = sc.room_rir_bank('mic', room, DIRECTIONS, DISTANCE, 300, device=DEV, baffle='rigid')
    assert np.array_equal(bank.rirs.view(np.uint32), direct.view(np.uint32))
    calls = []
    monkeypatch.setattr(rooms, '_rirs_hip_sphere', lambda *a, **k: calls.append(1))
    monkeypatch.setattr(rooms, 'HIP_ROOM', False)
    leg = sc.room_rir_bank('mic', room, DIRECTIONS, DISTANCE, 300, device=DEV, baffle='rigid')
    assert not calls
    holds('public torch', leg.rirs, 300)
    assert bank.azimuth.tolist() == [d[0] for d in DIRECTIONS] and bank.elevation.tolist() == [d[1] for d in DIRECTIONS] and bank.audio_format == 'mic'
    open_bank = sc.room_rir_bank('mic', room, DIRECTIONS, DISTANCE, 300, device=DEV)
    assert not np.allclose(open_bank.rirs[:, :, :64], bank.rirs[:, :, :64], atol=0.05)


# ---- the hand-off ----------------------------------------------------------------------------------------------------------------------
def test_a_rigid_bank_comes_with_its_spectra_and_renders():
    from salsa_amd import rooms, scenes as sc
    room = rooms.ShoeboxRoom(SIZE, beta=BETA)
    bank = rooms.room_rir_bank('mic', room, DIRECTIONS, DISTANCE, 700, device=DEV, baffle='rigid')
    assert list(bank._spectra) == [('cuda', 0)]
    pre = bank.spectra(DEV)
    fresh = sc.RirBank(bank.rirs, bank.azimuth, bank.elevation, 'mic')
    up = fresh.spectra(DEV)
    assert up.shape == pre.shape and torch.equal(up.view(torch.int32), pre.view(torch.int32))
    open_bank = rooms.room_rir_bank('mic', room, DIRECTIONS, DISTANCE, 700, device=DEV)
    pool = sc.synth_event_pool(4, 2, 1, max_s=0.8)
    scenes = sc.draw_scenes(1, pool, bank, 2 * 24000, 4, max_polyphony=2, gap_s=(0.1, 0.4))
    rigid, free = sc.render_scenes(scenes, pool, bank, device=DEV), sc.render_scenes(scenes, pool, open_bank, device=DEV)
    assert tuple(rigid.shape) == (1, 4, 2 * 24000) and bool(torch.isfinite(rigid).all()) and float(rigid.abs().max()) > 1e-3
    assert float((rigid - free).abs().max()) > 1e-2 * float(free.abs().max())
