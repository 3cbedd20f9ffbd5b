"""CPU tests of the octave-band rooms (salsa_amd/rooms.py): the filterbank, the banded image table, the composed
torch path (device='cpu') against the float64 restatement tests/room_bands_reference.py, per-band measurement and calibration on the
torch path, and the refusals.  Nothing here needs a GPU."""
import functools

import numpy as np
import pytest

import room_bands_reference as rb
import room_reference as rr

FS = 24000
SIZE, ARRAY = (3.1, 2.3, 2.7), (1.4, 1.1, 1.2)
BANDS3 = (250, 1000, 4000)
BETA3 = np.array([[0.9, 0.85, 0.8, 0.75, 0.7, 0.65], [0.7, 0.7, 0.6, 0.6, 0.5, 0.5], [0.4, 0.0, 0.5, 0.3, 0.45, 0.35]])
DIRECTIONS = ((-60, 20), (135, -35))
HALF, LENGTH = 64, 300


# ---- the filterbank ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('half', [16, 512, 1024])
def test_the_filters_sum_to_a_unit_impulse(half):
    from salsa_amd import rooms
    h = rooms.octave_filters(FS, half=half)
    assert h.dtype == np.float64 and h.shape == (7, 2 * half + 1)
    delta = np.zeros(2 * half + 1)
    delta[half] = 1.0
    assert np.abs(h.sum(axis=0) - delta).max() <= 1e-15
    assert np.array_equal(h, h[:, ::-1]) or np.abs(h - h[:, ::-1]).max() <= 1e-16      # linear phase: symmetric about the centre
    assert np.abs(h - rb.filters(FS, rb.OCTAVE_BANDS, half)).max() <= 1e-14            # the cosine sum of the reference


def test_defaults_and_other_band_sets():
    from salsa_amd import rooms, scenes
    assert rooms.OCTAVE_BANDS == (125, 250, 500, 1000, 2000, 4000, 8000) and scenes.OCTAVE_BANDS is rooms.OCTAVE_BANDS
    assert scenes.octave_filters is rooms.octave_filters
    assert rooms.octave_filters(FS).shape == (7, 2049)
    one = rooms.octave_filters(FS, (1000,), 16)
    assert one.shape == (1, 33) and one[0, 16] == 1.0 and np.abs(one).sum() <= 1.0 + 1e-15     # one band: the impulse itself
    h = rooms.octave_filters(FS, BANDS3, HALF)
    assert np.abs(h - rb.filters(FS, BANDS3, HALF)).max() <= 1e-14


def test_the_gains_are_reproduced_to_the_windows_smoothing():
    """The taps are the gains' inverse transform times a Hann window of 2 D + 3 points: their transform is G smoothed by the window's
    kernel, whose main lobe reaches fs / (D + 1) to either side (23.4 Hz at D = 1024) and whose side lobes lie below 10^(-31.5 / 20) =
    0.027 of its peak and alternate in sign.  Further than one main-lobe half width from every transition region of a band the smoothed
    gain therefore stays within 0.027 of G (0 or 1 there); inside a region it is only bounded by [0 - 0.027, 1 + 0.027]."""
    from salsa_amd import rooms
    D = 1024
    h = rooms.octave_filters(FS, half=D)
    n = 1 << 16
    f = np.arange(n // 2 + 1) * (FS / n)
    H = np.fft.rfft(np.roll(np.pad(h, ((0, 0), (0, n - h.shape[1]))), -D, axis=1), axis=1)
    assert np.abs(H.imag).max() <= 1e-12                                       # zero phase once the centre is at 0
    G = rb.gains(f, rb.OCTAVE_BANDS)
    lobe = 2.0 * FS / (2 * D + 2)
    flat = np.ones(len(f), bool)
    for fb in rb.OCTAVE_BANDS[:-1]:
        e = fb * np.sqrt(2.0)
        flat &= (f < e * 2 ** -0.25 - lobe) | (f > e * 2 ** 0.25 + lobe)
    assert flat[np.searchsorted(f, 120.0)] and flat[np.searchsorted(f, 250.0)] and flat.sum() > 0.6 * len(f)
    assert np.abs(H.real - G)[:, flat].max() <= 0.027
    assert H.real.min() >= -0.027 and H.real.max() <= 1.027
    assert np.abs(H.real.sum(axis=0) - 1.0).max() <= 1e-12                     # complementary at every frequency


# ---- the room and its image table ------------------------------------------------------------------------------------------------
def test_a_banded_room_and_its_image_table():
    from salsa_amd import rooms
    room = rooms.ShoeboxRoom(SIZE, beta=BETA3, array=ARRAY, bands=BANDS3, band_half=HALF)
    assert room.bands == (250.0, 1000.0, 4000.0) and room.beta.shape == (3, 6) and room.band_half == HALF and room.rt60 is None
    plain = rooms.ShoeboxRoom(SIZE, beta=BETA3[0], array=ARRAY)
    assert plain.bands is None and plain.beta.shape == (6,)
    d_max = 9.0
    images = rooms.room_images(room, d_max)
    N = len(images)
    assert images.amplitude.shape == (3, N) and images.band_table().shape == (9, N) and images.band_table().dtype == np.float64
    with pytest.raises(ValueError):
        images.table()
    # kept iff the distance rule holds and some band's amplitude is > 0: the union of the bands' own tables, in canonical order
    own = [rooms.room_images(rooms.ShoeboxRoom(SIZE, beta=BETA3[b], array=ARRAY), d_max) for b in range(3)]
    keys = sorted(set().union(*[set(map(tuple, np.concatenate([o.n, o.q], axis=1).tolist())) for o in own]))
    assert [tuple(r) for r in np.concatenate([images.n, images.q], axis=1).tolist()] == keys
    assert N == len(own[0]) > len(own[2])                                      # band 2 has a wall of beta 0: fewer images of its own
    for b in range(3):
        at = {tuple(k): a for k, a in zip(np.concatenate([own[b].n, own[b].q], axis=1).tolist(), own[b].amplitude)}
        assert np.array_equal(images.amplitude[b], [at.get(k, 0.0) for k in keys])
    assert (images.amplitude[2] == 0).any() and (images.amplitude > 0).any(axis=0).all()
    assert np.array_equal(images.band_table()[:6], own[0].table()[:6]) and np.array_equal(images.band_table()[6], own[0].table()[6])
    # K = 1 is today's table
    single = rooms.room_images(rooms.ShoeboxRoom(SIZE, beta=BETA3[:1], array=ARRAY, bands=(1000,)), d_max)
    assert np.array_equal(single.band_table(), own[0].table()) and np.array_equal(own[0].band_table(), own[0].table())
    # max_order applies to the shared table
    assert int(rooms.room_images(room, d_max, max_order=2).order.max()) == 2


def test_rt60_per_band_is_eyring_per_band():
    from salsa_amd import rooms
    rt = (0.5, 0.4, 0.3)
    room = rooms.ShoeboxRoom(SIZE, rt60=rt, bands=BANDS3)
    assert np.array_equal(room.rt60, rt) and room.band_half == rooms.BAND_HALF == 1024
    for b in range(3):
        assert np.array_equal(room.beta[b], np.full(6, rooms.eyring_beta(SIZE, rt[b])))
    assert np.array_equal(rooms.ShoeboxRoom(SIZE, beta=(0.9, 0.8, 0.7), bands=BANDS3).beta, np.repeat([[0.9], [0.8], [0.7]], 6, axis=1))


# ---- the torch path against float64 --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(fmt):
    out = []
    for direction in DIRECTIONS:
        src = rr.source(ARRAY, direction, 0.7)
        out.append(rb.room_response(SIZE, BETA3, BANDS3, HALF, FS, src, rr.receivers(fmt, ARRAY), fmt == 'foa', LENGTH)[:2])
    ref = np.stack([o[0] for o in out])
    yards = [np.stack([o[1][i] for o in out]) for i in (0, 1)]
    return ref, yards


@pytest.mark.parametrize('fmt', ['foa', 'mic'])
def test_the_torch_path_holds_the_float64_reference(fmt):
    from salsa_amd import rooms
    room = rooms.ShoeboxRoom(SIZE, beta=BETA3, array=ARRAY, bands=BANDS3, band_half=HALF)
    got, directions = rooms.room_rirs(fmt, room, DIRECTIONS, 0.7, LENGTH, device='cpu')
    got = got.numpy()
    ref, yards = _reference(fmt)
    assert got.shape == ref.shape == (2, 4, LENGTH) and got.dtype == np.float32 and directions.tolist() == [list(d) for d in DIRECTIONS]
    err, Y = float(np.abs(got - ref).max()), rb.yard_error(ref, yards)
    print('RATIO torch %s: err %.3e Y %.3e ratio %.2f peak %.3f' % (fmt, err, Y, err / Y, np.abs(ref).max()))
    assert 0.5 < np.abs(ref).max() < 2.0 and err <= rb.bound(ref, Y)
    bank = rooms.room_rir_bank(fmt, room, DIRECTIONS, 0.7, LENGTH, device='cpu')
    assert np.array_equal(bank.rirs, got) and bank.audio_format == fmt


@pytest.mark.parametrize('fmt', ['foa', 'mic'])
def test_equal_bands_give_the_broadband_room(fmt):
    """All seven bands carry the same walls: r_b = r for every b, so h = sum_j (sum_b h_b[j]) r[k + D - j] = r[k] + sum_j eps[j] r[k + D - j]
    with eps = sum_b fl32(h_b) - delta, which the test computes.  Against the broadband float32 response the torch path may differ by
    (a) that term, at most |eps|_1 max |r|, and (b) the rounding of its float32 merge: K (2 D + 1) products and as many additions, each
    within 2^-24 relative, on terms whose absolute sum per output is at most |h|_1 max |r| -- n 2^-24 |h|_1 max |r| with n = 2 K (2 D + 1)
    counted as tests/small_kernels_reference.py counts a sum's roundings, (c) one rounding of each band row against the broadband row
    does not arise: the rows are the same float32 numbers."""
    from salsa_amd import rooms
    beta = BETA3[0]
    plain = rooms.ShoeboxRoom(SIZE, beta=beta, array=ARRAY)
    banded = rooms.ShoeboxRoom(SIZE, beta=np.tile(beta, (7, 1)), array=ARRAY, bands=rooms.OCTAVE_BANDS, band_half=HALF)
    want = rooms.room_rirs(fmt, plain, DIRECTIONS, 0.7, LENGTH, device='cpu')[0].numpy()
    got = rooms.room_rirs(fmt, banded, DIRECTIONS, 0.7, LENGTH, device='cpu')[0].numpy()
    h32 = rooms.octave_filters(FS, half=HALF).astype(np.float32).astype(np.float64)
    eps = h32.sum(axis=0)
    eps[HALF] -= 1.0
    peak, n = float(np.abs(want).max()), 2 * 7 * (2 * HALF + 1)
    bound = (np.abs(eps).sum() + n * 2.0 ** -24 * np.abs(h32).sum()) * peak
    err = float(np.abs(got.astype(np.float64) - want).max())
    print('EQUAL BANDS %s: err %.3e (%.1e of the peak), bound %.3e' % (fmt, err, err / peak, bound))
    assert peak > 0.5 and err <= bound


# ---- measurement and calibration on the torch path -----------------------------------------------------------------------------
def test_per_band_measurement_is_the_broadband_measurement_of_the_band_signals():
    from salsa_amd import rooms
    room = rooms.ShoeboxRoom(SIZE, beta=BETA3, array=ARRAY, bands=BANDS3, band_half=HALF)
    bank = rooms.room_rir_bank("foa", room, DIRECTIONS, 0.7, 3000, device="cpu")
    got = rooms.rir_acoustics(bank.rirs, device='cpu', bands=BANDS3, band_half=HALF, edc=True)
    assert got.t20.shape == (2, 4, 3) and got.crossings.shape == (2, 4, 3, 5) and got.edc.shape == (2, 4, 3, 3000)
    y = rb.split(bank.rirs.reshape(8, 3000), rb.filters(FS, BANDS3, HALF).astype(np.float32)).astype(np.float32).reshape(2, 4, 3, 3000)
    for b in range(3):
        own = rooms.rir_acoustics(y[:, :, b], device='cpu')
        assert np.allclose(got.t20[..., b], own.t20, rtol=1e-3, equal_nan=True) and np.allclose(got.energy[..., b], own.energy, rtol=1e-4)
    assert got.t20[0, 0, 0] > got.t20[0, 0, 2] > 0                             # the absorbing band decays faster
    via_bank = bank.acoustics(device='cpu', bands=BANDS3, band_half=HALF)
    assert np.array_equal(via_bank.params, got.params, equal_nan=True)
    plain = rooms.rir_acoustics(bank.rirs, device='cpu')
    assert plain.t20.shape == (2, 4)


def test_calibration_per_band_on_the_torch_path():
    from salsa_amd import rooms
    target = (0.16, 0.12)
    room = rooms.calibrate_room((3.0, 2.5, 2.2), rt60=target, bands=(500, 2000), band_half=128, length=3600, device='cpu', directions=((0, 0), (100, 10)),
                                distance=0.6)
    c = room.calibration
    assert room.bands == (500.0, 2000.0) and room.beta.shape == (2, 6) and room.band_half == 128
    assert c['target'].tolist() == list(target) and c['realised'].shape == (2,) and np.all(np.abs(c['realised'] / c['target'] - 1) <= 0.01)
    assert c['evaluations'] == len(c['beta_history']) == len(c['realised_history']) <= 8 and c['beta_history'][-1].shape == (2, 6)
    assert np.array_equal(c['beta_history'][-1], room.beta) and c['probes'].shape == (2, 2) and c['headroom_db'].min() >= 15.0
    assert np.all(c['beta_history'][0] == [[rooms.eyring_beta((3.0, 2.5, 2.2), t)] * 6 for t in target])
    with pytest.raises(ValueError, match='one per band'):
        rooms.calibrate_room((3.0, 2.5, 2.2), rt60=0.2, bands=(500, 2000), device='cpu')


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from salsa_amd import rooms
    banded = rooms.ShoeboxRoom(SIZE, beta=BETA3, array=ARRAY, bands=BANDS3, band_half=HALF)
    for call in (lambda: rooms.room_rirs('mic', banded, DIRECTIONS, 0.7, LENGTH, device='cpu', baffle='rigid'),
                 lambda: rooms.room_rir_bank('mic', banded, DIRECTIONS, 0.7, LENGTH, device='cpu', baffle='rigid'),
                 lambda: rooms.room_geometry('mic', banded, DIRECTIONS, 0.7, LENGTH, baffle='rigid'),
                 lambda: rooms.calibrate_room(SIZE, rt60=(0.3, 0.3, 0.3), bands=BANDS3, audio_format='mic', baffle='rigid', device='cpu')):
        with pytest.raises(ValueError, match='bands'):
            call()
    nine = tuple(100 * 1.5 ** i for i in range(9))
    for bad in (nine, (), (500, 250), (250, 250), (-1, 250), (4000, 9000, 16000), ((250, 500),)):
        with pytest.raises(ValueError):
            rooms.ShoeboxRoom(SIZE, beta=0.5 * np.ones(len(np.ravel(bad))), bands=bad)
        with pytest.raises(ValueError):
            rooms.octave_filters(FS, bad)
    with pytest.raises(ValueError):
        rooms.rir_acoustics(np.zeros((1, 1, 64), np.float32), device='cpu', bands=nine)
    for beta in (0.5, np.ones(6) * 0.5, np.ones((3, 5)) * 0.5, np.ones((2, 6)) * 0.5, np.ones((3, 6)) * 1.5):
        with pytest.raises(ValueError):
            rooms.ShoeboxRoom(SIZE, beta=beta, bands=BANDS3)
    for rt in (0.3, (0.3, 0.3), (0.3, 0.3, -0.1)):
        with pytest.raises(ValueError):
            rooms.ShoeboxRoom(SIZE, rt60=rt, bands=BANDS3)
    for half in (0, 2049, 1.5):
        with pytest.raises(ValueError):
            rooms.octave_filters(FS, half=half)
        with pytest.raises(ValueError):
            rooms.ShoeboxRoom(SIZE, beta=BETA3, bands=BANDS3, band_half=half)
    with pytest.raises(ValueError):
        rooms.ShoeboxRoom(SIZE, beta=np.ones((3, 6)) * 0.5)                    # (K, 6) without bands stays refused
