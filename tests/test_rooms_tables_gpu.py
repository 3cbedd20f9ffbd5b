"""GPU tests of salsa_room_rirs (salsa_amd/csrc/room_rir.hip) on image tables BUILT BY HAND (tests/room_tables.py),
against the table-level float64 reference room_reference.response_of_table.  No physical room fills a wave or a chunk of the kernel's
compaction (the densest real table of tests/test_rooms_gpu.py keeps about 30 of 256 images per chunk); these tables do.

  compaction   hit masks with full waves (64), full chunks (256), single lanes, empty chunks, the last index alone, none; each for FOA
               and for four omni receivers.  Held: the float64 bound max |got - ref64| <= 4 Y + ulp32(max |ref64|) (section 9j's rule, Y
               from the float32 yardstick in table order and reversed, reference and Y from room_reference alone); SQUEEZE INVARIANCE --
               the bits of the table with its misses taken out; +0.0 bits outside every support.
  edges        delays in (-16, 4) with t0 > 0; shorter lengths as bit-exact prefixes on the device; one, two and three omni receivers.
  order        tables with exact arithmetic (fs / c = 1, whole distances, fraction 0): a tap's bits are those of a sequential np.float32
               sum IN TABLE ORDER -- 1 then 4096 x 2^-25 is 1.0f, the reverse 1 + 2^-13 --, and every neighbouring tap inside the
               supports is +0.0: the exact zero of sinpif at whole delays.  This rests on the device's float64 sqrt returning n for
               n^2 (no fast-math flag is set), which these tests measure: it does, on an MI355X.
  offsets      a 2^31 + 65536-float FOA output, checked on the device.
Every output lies inside NaN guard bands, 4-byte aligned only, every element written.  Measured ratios error / Y are in MEASURED."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import room_reference as rr
import room_tables as rt
from salsa_amd import _lib

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARD = 67                                                                     # floats on either side of the output: odd
FACTOR = 4.0
MEASURED = """ratio (error) / Y per case, on one MI355X (the bound is 4 Y + one float32 ulp of the largest |ref64|); errors 4e-9 .. 9e-6 on sums of
up to 1025 images with coefficients of order 1
  table             foa    omni (4 receivers)
  all_1             0.39   0.77
  all_63            1.22   1.03
  all_64            0.82   0.76
  all_65            1.00   0.60
  all_255           0.51   0.51
  all_256           0.49   0.66
  all_257           1.17   0.94
  all_1023          0.81   1.13
  all_1024          0.92   0.92
  all_1025          1.00   0.55
  chunk1_miss       0.69   0.72
  lane0             1.73   1.72
  lane63            0.71   1.01
  waves_0_2         1.28   1.21
  alternating       1.03   0.85
  last_only         0.14   0.89
  none              -      -      (error 0, Y 0)
  negative delays   0.88   0.82
  alternating with 1, 2, 3 omni receivers: 1.03, 1.03, 0.85
No case needed more than 1.73.  The exact tables: the device's float64 sqrt returned n for every n^2 used (20 .. 16019, and the whole
triples' lengths 29 .. 290), so every order check holds bit for bit, the exact zeros beside a whole delay included: tap 40 reads 1.0
in table order and 1.0001220703125 = 1 + 2^-13 reversed.
Kernels broken by hand, in bounds, run against this file and tests/test_rooms_gpu.py (not part of the suite): the compacted entries read
backwards, the chunks walked backwards, the waves' counts summed in reverse -- three wrong ORDERS -- pass every float64 bound of both
files and fail here on squeeze invariance (lane0, lane63, waves_0_2, alternating), both exact order tests and the prefixes; the lane mask
cut to 32 bits fails nearly everything in both files; sin(pi x) per tap in place of the addition theorem fails only the exact
tables' zeros; omni rows stored in reverse fail every omni case; an order that depends on the number of tap blocks fails only the prefixes."""


def _run_device(table, src_rows, receivers, foa, fs_over_c, length):
    """salsa_room_rirs on the tables as they are, the output inside NaN guard bands -> device tensor (R, 4 or M, length), a view"""
    table, src_rows = np.ascontiguousarray(table, np.float64), np.ascontiguousarray(src_rows, np.float64).reshape(-1, 5)
    receivers = np.ascontiguousarray(receivers, np.float64).reshape(-1, 3)
    R, Cn = len(src_rows), 4 if foa else len(receivers)
    n = R * Cn * length
    buf = torch.full((n + 2 * GUARD,), float('nan'), dtype=torch.float32, device=DEV)
    d_table, d_sources = torch.from_numpy(table).to(DEV), torch.from_numpy(src_rows).to(DEV)
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc = _lib.load().salsa_room_rirs(p(table), C.c_void_p(d_table.data_ptr()), table.shape[1], p(src_rows), C.c_void_p(d_sources.data_ptr()), R,
                                     p(receivers), len(receivers), int(foa), fs_over_c, length,
                                     C.c_void_p(buf[GUARD:].data_ptr()), C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all()), 'a guard band was written'
    return buf[GUARD:GUARD + n].view(R, Cn, length)


def _run(table, src, receivers, foa, fs_over_c=rt.FS_OVER_C, length=rt.LENGTH):
    """one source src = (position, t0, g) -> numpy (4 or M, length)"""
    out = _run_device(table, rt.source_row(src), receivers, foa, fs_over_c, length)
    assert not bool(torch.isnan(out).any()), 'an output element was not written'
    return out[0].cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _receivers(fmt):
    return rt.RECEIVER[None] if fmt == 'foa' else rt.RECEIVERS


def _holds(what, got, reference):
    """got (C, length) against reference = (ref64, yardsticks, reached), rows beyond got's left out -> the ratio error / Y"""
    ref, yards, reached = (a[:len(got)] if isinstance(a, np.ndarray) else [y[:len(got)] for y in a] for a in reference)
    assert got.shape == ref.shape and np.isfinite(got).all()
    err = float(np.abs(got.astype(np.float64) - ref).max())
    Y = max(float(np.abs(y.astype(np.float64) - ref).max()) for y in yards)
    floor = rr.ulp32(np.abs(ref).max())
    print('RATIO %s: err %.3e Y %.3e floor %.3e ratio %s' % (what, err, Y, floor, '%.2f' % (err / Y) if Y else '-'))
    assert err <= FACTOR * Y + floor, '%s: error %.3e > %g x %.3e + %.3e' % (what, err, FACTOR, Y, floor)
    assert not _bits(got[~reached]).any(), 'a tap outside every support is +0.0'
    return err / Y if Y else 0.0


# ---- compaction patterns -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mask_reference(name, fmt):
    return rr.table_reference(rt.built_table(rt.MASKS[name]), rt.source(), _receivers(fmt), fmt == 'foa', rt.LENGTH, rt.FS_OVER_C)


@pytest.mark.parametrize('fmt', ['foa', 'omni'])
@pytest.mark.parametrize('name', list(rt.MASKS))
def test_compaction_patterns(name, fmt):
    mask, foa = rt.MASKS[name], fmt == 'foa'
    table = rt.built_table(mask)
    got = _run(table, rt.source(), _receivers(fmt), foa)
    _holds('%s %s' % (name, fmt), got, _mask_reference(name, fmt))
    if not mask.any():
        assert not _bits(got).any(), 'no image: +0.0 everywhere'
        return
    assert np.abs(got).max() > 0.01 and (mask.sum() < 200 or np.abs(got[:, 256:]).max() > 0.01)      # the short tap block carries taps too
    if not mask.all():
        squeezed = _run(table[:, mask], rt.source(), _receivers(fmt), foa)
        assert np.array_equal(_bits(squeezed), _bits(got)), 'the misses changed a bit'


# ---- negative delays, prefixes, receivers --------------------------------------------------------------------------------------
@pytest.mark.parametrize('fmt', ['foa', 'omni'])
def test_delays_below_zero(fmt):
    table, src = rt.negative_delay_table(), rt.source(t0=40.0)
    reference = rr.table_reference(table, src, _receivers(fmt), fmt == 'foa', rt.LENGTH, rt.FS_OVER_C)
    got = _run(table, src, _receivers(fmt), fmt == 'foa')
    _holds('negative delays %s' % fmt, got, reference)
    assert np.abs(got[:, :4]).max() > 0.1 and not got[:, 24:].any()                   # (the other receivers lie up to 3 taps away)


ROOM = dict(size=(3.1, 2.3, 2.7), beta=(0.9, 0.85, 0.8, 0.75, 0.7, 0.65), array=(1.4, 1.1, 1.2))
DIRECTIONS = ((-60, 20), (135, -35), (0, 90))


@pytest.mark.parametrize('fmt', ['foa', 'mic'])
def test_a_shorter_response_is_a_prefix_on_the_device(fmt):
    """a real room's table for 769 taps: the lengths 255, 256, 257 and 300 give the first taps of the 769-tap response bit for bit, from
    the same table and from the (shorter) table of their own length alike"""
    from salsa_amd import rooms
    room = rooms.ShoeboxRoom(ROOM['size'], beta=ROOM['beta'], array=ROOM['array'])
    fs_over_c, foa = room.fs / room.c, fmt == 'foa'
    _, sources, receivers, d_max = rooms.room_geometry(fmt, room, DIRECTIONS, 0.7, 769)
    table = rooms.room_images(room, d_max).table()
    full = _run_device(table, sources, receivers, foa, fs_over_c, 769).cpu().numpy()
    assert np.isfinite(full).all() and np.abs(full[:, :, 300:]).max() > 1e-3
    for length in (255, 256, 257, 300):
        short = _run_device(table, sources, receivers, foa, fs_over_c, length).cpu().numpy()
        assert np.array_equal(_bits(short), _bits(full[:, :, :length])), 'length %d is not a prefix' % length
        _, sources_l, _, d_max_l = rooms.room_geometry(fmt, room, DIRECTIONS, 0.7, length)
        own = rooms.room_images(room, d_max_l).table()
        assert np.array_equal(sources_l, sources) and own.shape[1] < table.shape[1]
        short = _run_device(own, sources, receivers, foa, fs_over_c, length).cpu().numpy()
        assert np.array_equal(_bits(short), _bits(full[:, :, :length])), 'length %d from its own table is not a prefix' % length


@pytest.mark.parametrize('M', [1, 2, 3])
def test_one_two_and_three_omni_receivers(M):
    """row m is the row of the four-receiver run, for a second source too (its g doubled: exactly twice the first)"""
    name = 'alternating'
    table, src = rt.built_table(rt.MASKS[name]), rt.source()
    rows = np.concatenate([rt.source_row(src), rt.source_row((src[0], src[1], 2.0 * src[2]))])
    four = _run_device(table, rows, rt.RECEIVERS, False, rt.FS_OVER_C, rt.LENGTH).cpu().numpy()
    got = _run_device(table, rows, rt.RECEIVERS[:M], False, rt.FS_OVER_C, rt.LENGTH).cpu().numpy()
    assert got.shape == (2, M, rt.LENGTH) and np.isfinite(got).all()
    _holds('%d receivers' % M, got[0], _mask_reference(name, 'omni'))
    assert np.array_equal(_bits(got), _bits(four[:, :M])), 'a row depends on the number of receivers'
    assert np.array_equal(_bits(got[1]), _bits(np.float32(2.0) * got[0])) and np.abs(got[0]).max(axis=1).min() > 0.01


# ---- table order, exactly ------------------------------------------------------------------------------------------------------
def _exact_run(table, g, foa):
    return _run(table, rt.exact_source(g), rt.EXACT_RECEIVER, foa, fs_over_c=1.0)


@pytest.mark.parametrize('fmt', ['foa', 'omni'])
def test_big_first_and_small_first(fmt):
    """1, then 4096 x 2^-25 over 17 chunks, all on tap 40 (shift (40, 0, 0): W and X carry it, Y and Z nothing): exactly 1.0f in table
    order, exactly 1 + 2^-13 in the reversed order; every other tap, inside the supports or not, is +0.0"""
    foa, table = fmt == 'foa', rt.big_first_table()
    for tab, value in ((table, 1.0), (table[:, ::-1], 1.0 + 2.0 ** -13)):
        got = _exact_run(tab, float(rt.BIG_TAP), foa)
        want = np.zeros_like(got)
        want[[0, 3] if foa else [0], rt.BIG_TAP] = np.float32(value)
        print('ORDER %s: tap %d = %r (W), want %r' % (fmt, rt.BIG_TAP, float(got[0, rt.BIG_TAP]), value))
        assert _bits(got[0, rt.BIG_TAP]) == _bits(np.float32(value)), 'the sum did not run in table order'
        assert np.array_equal(_bits(got), _bits(want)), 'a tap beside a whole delay is not +0.0'


@pytest.mark.parametrize('fmt', ['foa', 'omni'])
def test_random_amplitudes_sum_in_table_order(fmt):
    """1000 images on the taps 29, 33, 45, 261, 290, off the axes too ((12, 16, 21) and its like, signed and permuted): every channel of
    every tap has the bits of the sequential np.float32 sum of float32(g A / d u_c) in table order"""
    foa = fmt == 'foa'
    table, _ = rt.random_exact_table()
    for tab in (table, table[:, ::-1]):
        want = rt.sequential_float32(tab, 29.0, rt.LENGTH)[:4 if foa else 1]
        got = _exact_run(tab, 29.0, foa)
        assert np.array_equal(_bits(got), _bits(want)), 'taps %s differ' % sorted(set(np.nonzero(_bits(got) != _bits(want))[1].tolist()))
    assert not np.array_equal(rt.sequential_float32(table, 29.0, rt.LENGTH), rt.sequential_float32(table[:, ::-1], 29.0, rt.LENGTH))


# ---- offsets past 2^31 ---------------------------------------------------------------------------------------------------------
def test_offsets_past_two_to_the_31():
    """FOA, 16384 taps, 32769 sources: 2^31 + 65536 output floats (8.6 GB).  One image, the exact geometry: source r at (d_r, 0, 0), d_r =
    20 + r mod 16000, g = d_r, so W and X of source r are 1.0f at tap d_r and +0.0 elsewhere, Y and Z +0.0.  Checked on the device."""
    R, length = 32769, 16384
    assert R * 4 * length == (1 << 31) + 65536
    free = torch.cuda.mem_get_info()[0]
    assert free > 10 * 2 ** 30, 'this test wants 10 GB of device memory'
    d = 20 + np.arange(R) % 16000
    rows = np.zeros((R, 5))
    rows[:, 0] = rows[:, 4] = d
    out = _run_device(rt.exact_table([(0, 0, 0)], [1.0]), rows, rt.EXACT_RECEIVER, True, 1.0, length)
    bits = out.view(torch.int32)
    one = int(np.float32(1.0).view(np.int32))
    at = torch.from_numpy(d).to(DEV)
    nonzero = 0
    for lo in range(0, R, 2048):
        part, idx = bits[lo:lo + 2048], at[lo:lo + 2048, None]
        for ch in (0, 3):
            assert bool((part[:, ch].gather(1, idx) == one).all()), 'sources %d ..: channel %d is not 1.0f at its tap' % (lo, ch)
        nonzero += int(torch.count_nonzero(part))                              # NaN (not written) and -0.0 count as well
    assert nonzero == 2 * R, '%d non-zero words, expected %d' % (nonzero, 2 * R)
    want = np.zeros((4, length), np.float32)
    want[[0, 3], d[-1]] = 1.0
    assert np.array_equal(_bits(out[-1].cpu().numpy()), _bits(want)), 'the last source, past 2^31'
    del out, bits
    torch.cuda.empty_cache()
