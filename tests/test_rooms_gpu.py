"""GPU tests of the shoebox image-source responses (salsa_amd/csrc/room_rir.hip, salsa_amd/rooms.py) against the
float64 restatement of tests/room_reference.py.

Bound of every comparison with float64, per source and format: max |got - ref64| <= 4 Y + ulp32(max |ref64|), Y the larger error of
the float32 yardstick (float64 geometry, float32 from the tap argument on, float32 accumulation) summed in table order and in
reversed table order: section 9j's convention.  The small room is (3.1, 2.3, 2.7) m with six distinct reflection coefficients, the
array off centre, sources at 0.7 m towards (-60, 20), (135, -35) and (0, 90); response lengths 1, 2 H + 1 and both sides of every
multiple of the kernel's tap block (256) up to three blocks.  A reference is computed once, at the longest length of its family (a
response is the prefix of a longer one), and shared.  Measured ratios error / Y are in MEASURED below."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import room_reference as rr
from salsa_amd import _lib

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARD = 67                                                                     # floats on either side of the output: odd, so `out` is 4-byte aligned only
SIZE, BETA, ARRAY = (3.1, 2.3, 2.7), (0.9, 0.85, 0.8, 0.75, 0.7, 0.65), (1.4, 1.1, 1.2)
DIRECTIONS = ((-60, 20), (135, -35), (0, 90))
BLOCK = 256
LENGTHS = [1, 2 * rr.H + 1] + [m * BLOCK + e for m in (1, 2, 3) for e in (-1, 0, 1)]
FACTOR = 4.0
MEASURED = """largest ratio (error) / Y over the sources of a case, on one MI355X; HIP: the kernel, torch: the SALSA_HIP_ROOM=0 leg on the device
  case                          HIP foa   HIP mic   torch foa   torch mic
  edges, length 1               0.00      1.05      -           -
  edges, lengths 33 .. 769      2.17      1.29      -           -          (every length alike: the largest error sits at the direct peak)
  near                          0.49      7.63*     1.00        7.63*
  cut_end                       2.18      1.29      1.00        1.00
  dead                          2.17      1.29      1.00        1.00
  one_wall                      1.61      1.00      1.00        1.00
  order0, order1, order3        2.17      1.29      1.00        1.00
  (* the source 8 mm from capsule 2: a peak of 4.4, error 5.49e-7 = 1.15 ulp of it from the kernel and the torch leg alike, against a
  yardstick that happened to land 0.15 ulp from the float64 value (Y = 7.2e-8); the error is below 4 Y + the one-ulp floor of 4.77e-7,
  which is what admits it.  No other case needed more than 2.2.  The torch leg is the yardstick's arithmetic, hence its 1.00.)
  end to end: 15853 non-zero bins (the oracle on the float64 render: 15853), largest deviation from the label 1.24e-6."""

# family -> (beta, directions, distance, length, keywords of room_geometry / room_images)
FAMILIES = {
    'near': (BETA, DIRECTIONS[:2], 0.05, 300, dict(align_direct=False)),       # supports cut at tap 0, 1 / d = 20
    'cut_end': ((0.0,) * 6, DIRECTIONS, 0.7, 20, {}),                          # the direct support (taps 1 .. 32) cut at the end
    'dead': ((0.0,) * 6, DIRECTIONS, 0.7, 300, {}),
    'one_wall': ((0.5, 0.0, 0.0, 0.0, 0.0, 0.0), DIRECTIONS, 0.7, 400, dict(align_direct=False, normalize_direct=False)),
    'order0': (BETA, DIRECTIONS, 0.7, 300, dict(max_order=0)),
    'order1': (BETA, DIRECTIONS, 0.7, 300, dict(max_order=1)),
    'order3': (BETA, DIRECTIONS, 0.7, 300, dict(max_order=3)),
}


@functools.lru_cache(maxsize=None)
def _reference(fmt, beta, direction, distance, length, align_direct=True, normalize_direct=True, max_order=None):
    """-> (ref64, [yardstick in table order, reversed], reached), each (C, length); shared by every test of the family, never written"""
    src = rr.source(ARRAY, direction, distance, align_direct, normalize_direct)
    imgs = rr.images(SIZE, beta, rr.d_max_of(length, src[1]), max_order)
    recs, foa = rr.receivers(fmt, ARRAY), fmt == 'foa'
    ref, reached = rr.response(imgs, SIZE, src, recs, foa, length)
    yards = [rr.response(imgs, SIZE, src, recs, foa, length, f32=True, reverse=rev)[0] for rev in (False, True)]
    for a in [ref, reached] + yards:
        a.setflags(write=False)
    return ref, yards, reached


def _tables(fmt, beta, directions, distance, length, max_order=None, **kw):
    from salsa_amd import rooms
    room = rooms.ShoeboxRoom(SIZE, beta=beta, array=ARRAY)
    _, sources, receivers, d_max = rooms.room_geometry(fmt, room, directions, distance, length, **kw)
    return rooms.room_images(room, d_max, max_order).table(), sources, receivers


def _run(fmt, beta, directions, distance, length, hip=True, **kw):
    """salsa_room_rirs (or the torch leg) on the public tables, the output inside NaN guard bands -> numpy (R, 4, length)"""
    from salsa_amd import rooms
    table, sources, receivers = _tables(fmt, beta, directions, distance, length, **kw)
    if not hip:
        return rooms._rirs_torch(table, sources, receivers, fmt == 'foa', rr.FS / rr.SOUND_SPEED, length, torch.device(DEV)).cpu().numpy()
    R, n = len(sources), len(sources) * 4 * length
    buf = torch.full((n + 2 * GUARD,), float('nan'), dtype=torch.float32, device=DEV)
    d_table, d_sources = torch.from_numpy(table).to(DEV), torch.from_numpy(sources).to(DEV)
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc = _lib.load().salsa_room_rirs(p(table), C.c_void_p(d_table.data_ptr()), table.shape[1], p(sources), C.c_void_p(d_sources.data_ptr()), R,
                                     p(receivers), len(receivers), int(fmt == 'foa'), rr.FS / rr.SOUND_SPEED, length,
                                     C.c_void_p(buf[GUARD:].data_ptr()), C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all()), 'a guard band was written'
    out = buf[GUARD:GUARD + n].view(R, 4, length)
    assert not bool(torch.isnan(out).any()), 'an output element was not written'
    return out.cpu().numpy()


def _holds(what, got, fmt, beta, directions, distance, length, full=None, **kw):
    """every source of `got` against the shared reference (computed at `full` taps, cut to `length`) -> the largest ratio error / Y"""
    worst = 0.0
    for r, direction in enumerate(directions):
        ref, yards, reached = (a[..., :length] if isinstance(a, np.ndarray) else [y[:, :length] for y in a]
                               for a in _reference(fmt, tuple(beta), direction, distance, full or length, **kw))
        err = float(np.abs(got[r].astype(np.float64) - ref).max())
        Y = max(float(np.abs(y.astype(np.float64) - ref).max()) for y in yards)
        floor = rr.ulp32(np.abs(ref).max())
        print('RATIO %s %s len %d source %d: err %.3e Y %.3e floor %.3e ratio %s' % (what, fmt, length, r, err, Y, floor, '%.2f' % (err / Y) if Y else '-'))
        assert np.isfinite(got[r]).all()
        assert err <= FACTOR * Y + floor, '%s %s source %d: error %.3e > %g x %.3e + %.3e' % (what, fmt, r, err, FACTOR, Y, floor)
        outside = ~reached
        assert np.array_equal(got[r][outside].view(np.uint32), np.zeros(int(outside.sum()), np.uint32)), 'a tap outside every support is +0.0'
        worst = max(worst, err / Y if Y else 0.0)
    return worst


# ---- the kernel against float64 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fmt', ['foa', 'mic'])
@pytest.mark.parametrize('length', LENGTHS)
def test_kernel_against_float64_at_the_tap_block_edges(length, fmt):
    got = _run(fmt, BETA, DIRECTIONS, 0.7, length)
    _holds('edges', got, fmt, BETA, DIRECTIONS, 0.7, length, full=max(LENGTHS))
    if length >= 2 * rr.H + 1:
        assert np.abs(got[:, 0]).max() > 0.5                                    # the direct path, normalised to 1 on W / the capsules


@pytest.mark.parametrize('fmt', ['foa', 'mic'])
@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_kernel_against_float64_families(family, fmt, monkeypatch):
    beta, directions, distance, length, kw = FAMILIES[family]
    got = _run(fmt, beta, directions, distance, length, **kw)
    _holds(family, got, fmt, beta, directions, distance, length, **kw)
    assert np.abs(got).max() > 0.5
    # the composed torch leg of SALSA_HIP_ROOM=0 on the device meets the same bound (it is not promised bit-equal)
    leg = _run(fmt, beta, directions, distance, length, hip=False, **kw)
    _holds(family + ' torch', leg, fmt, beta, directions, distance, length, **kw)


# ---- exact properties ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fmt', ['foa', 'mic'])
def test_exact_properties(fmt):
    length = 2 * BLOCK + 44
    batch = _run(fmt, BETA, DIRECTIONS, 0.7, length)
    assert np.array_equal(_run(fmt, BETA, DIRECTIONS, 0.7, length).view(np.uint32), batch.view(np.uint32)), 'two runs give equal bits'
    for r in range(3):
        alone = _run(fmt, BETA, DIRECTIONS[r:r + 1], 0.7, length)
        assert np.array_equal(alone[0].view(np.uint32), batch[r].view(np.uint32)), 'a source alone gives the bits it has in a batch'
    zero = _run(fmt, BETA, DIRECTIONS, 0.7, length, max_order=0)
    dead = _run(fmt, (0.0,) * 6, DIRECTIONS, 0.7, length)
    assert np.array_equal(zero.view(np.uint32), dead.view(np.uint32)) and np.abs(zero).max() > 0.5, 'max_order = 0 is the dead room'
    assert not np.array_equal(zero, batch)


def test_the_public_path_runs_the_kernel_and_the_switch_leaves_it(monkeypatch):
    from salsa_amd import rooms, scenes as sc
    room = rooms.ShoeboxRoom(SIZE, beta=BETA, array=ARRAY)
    for fmt in ('foa', 'mic'):
        bank = sc.room_rir_bank(fmt, room, DIRECTIONS, 0.7, 300, device=DEV)
        assert np.array_equal(bank.rirs.view(np.uint32), _run(fmt, BETA, DIRECTIONS, 0.7, 300).view(np.uint32))
        monkeypatch.setattr(rooms, 'HIP_ROOM', False)
        leg = sc.room_rir_bank(fmt, room, DIRECTIONS, 0.7, 300, device=DEV)
        monkeypatch.setattr(rooms, 'HIP_ROOM', True)
        _holds('public torch', leg.rirs, fmt, BETA, DIRECTIONS, 0.7, 300)
        assert bank.azimuth.tolist() == [-60, 135, 0] and bank.elevation.tolist() == [20, -35, 90] and bank.audio_format == fmt


# ---- prefilled spectra ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fmt', ['foa', 'mic'])
def test_a_generated_bank_comes_with_the_spectra_of_the_upload_path(fmt):
    from salsa_amd import rooms, scenes as sc
    bank = rooms.room_rir_bank(fmt, rooms.ShoeboxRoom(SIZE, beta=BETA, array=ARRAY), DIRECTIONS, 0.7, 700, device=DEV)
    assert list(bank._spectra) == [('cuda', 0)]
    pre = bank.spectra(DEV)
    assert pre is bank._spectra[('cuda', 0)]
    fresh = sc.RirBank(bank.rirs, bank.azimuth, bank.elevation, fmt)
    assert not fresh._spectra
    up = fresh.spectra(DEV)
    assert up.shape == pre.shape and torch.equal(up.view(torch.int32), pre.view(torch.int32))


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def test_an_anechoic_room_puts_its_label_into_every_bin(oracle):
    """render a source of an all-beta-0 room 1.5 m towards (-130, 40), extract with SalsaExtractor, read the direction back.  1e-5 is the
    feature path's parity bar to the oracle; m = 2.08e-7 is the largest deviation the oracle produced on the CPU from the float32
    yardstick response (table and reversed order alike) rendered in float64 (1.61e-7 from the float64 response rounded to float32),
    times 4 as above.  The count of non-zero bins must reach 0.9 x the oracle's on the float64 render (15853 on the CPU)."""
    import scene_reference as sr
    from salsa_amd import rooms, scenes as sc
    from salsa_amd.extractor import SalsaExtractor
    from salsa_amd.synth import _ar1
    size, direction, length = (6.0, 5.0, 3.2), (-130, 40), 64
    pool = sc.EventPool([(0.1 * _ar1(np.random.RandomState(3).randn(24000))).astype(np.float32)], [2])
    bank = rooms.room_rir_bank('foa', rooms.ShoeboxRoom(size, beta=0.0), [(70, -20), direction], 1.5, length, device=DEV)
    scenes = sc.Scenes.from_items(48000, [[(0, 1, 9000, 0.8, 0)]], pool, bank)
    audio = sc.render_scenes(scenes, pool, bank)
    feat = SalsaExtractor(audio_format='foa', fmax_doa=9000, device=torch.device(DEV)).extract(audio)[0].cpu().numpy()
    src = rr.source(0.5 * np.array(size), direction, 1.5)
    ref = rr.response(rr.images(size, (0.0,) * 6, rr.d_max_of(length, src[1])), size, src, rr.receivers('foa', 0.5 * np.array(size)), True, length)[0]
    ref_bank = sc.RirBank(np.stack([ref, ref]).astype(np.float32), [70, -130], [-20, 40], 'foa')
    ref_feat = oracle.extract_salsa(sr.render64(scenes, pool, ref_bank, 48000)[0].astype(np.float32), audio_format='foa', fmax_doa=9000)
    nz, ref_nz = (feat[4:] != 0).any(axis=0), (ref_feat[4:] != 0).any(axis=0)
    x, y, z = sc._unit(*direction)
    dev = np.abs(feat[4:][:, nz] - np.array([y, z, x])[:, None]).max()
    print('%d non-zero bins (oracle on the float64 render: %d), largest deviation %.3g' % (nz.sum(), ref_nz.sum(), dev))
    assert dev <= 1e-5 + 4 * 2.08e-7
    assert nz.sum() >= 0.9 * ref_nz.sum() and ref_nz.sum() > 10000


def test_a_reverberant_bank_feeds_moving_scenes_and_a_training_step():
    from salsa_amd import rooms, scenes as sc
    from salsa_amd.crnn.train import Trainer
    from salsa_amd.dataset import GpuFeatureBank
    from salsa_amd.extractor import SalsaExtractor
    NC, n_samples = 12, 8 * 24000
    pool = sc.synth_event_pool(NC, 2, 1, max_s=1.2)
    rbank = rooms.room_rir_bank('foa', rooms.ShoeboxRoom(SIZE, beta=BETA, array=ARRAY), [(a, 10) for a in range(-180, 180, 30)], 0.7, 1200,
                                device=DEV)
    assert rbank.rirs.shape == (12, 4, 1200) and np.abs(rbank.rirs[:, :, 600:]).max() > 1e-3      # a tail, not a tap
    scenes = sc.draw_scenes(2, pool, rbank, n_samples, 4, max_polyphony=3, gap_s=(0.1, 0.8), moving=0.5)
    assert scenes.has_trajectories
    ex = SalsaExtractor(audio_format='foa', fmax_doa=9000, device=torch.device(DEV))
    bank = GpuFeatureBank(ex, n_classes=NC, label_format='classwise')
    audio = sc.add_scenes(bank, scenes, pool, rbank)
    assert tuple(audio.shape) == (2, 4, n_samples) and bool(torch.isfinite(audio).all()) and bank.clip_len == [640, 640]
    bank.fit_scaler()
    bank.finalize()
    for b in range(2):
        sed, doa = sc.scene_labels(scenes[b], 80, NC, 'classwise')
        assert sed.sum() > 0
        assert np.array_equal(bank.sed_all[80 * b:80 * (b + 1)].cpu().numpy().view(np.uint32), sed.view(np.uint32))
        assert np.array_equal(bank.doa_all[80 * b:80 * (b + 1)].cpu().numpy().view(np.uint32), doa.view(np.uint32))
    x, sed, doa, names = bank.batch([0, 1])
    assert tuple(x.shape) == (2, 7, 640, 200) and tuple(sed.shape) == (2, 80, NC) and tuple(doa.shape) == (2, 80, 3 * NC)
    losses = Trainer('cuda', seed=3).train_step(x, sed, doa)
    assert all(bool(torch.isfinite(v)) for v in losses)
