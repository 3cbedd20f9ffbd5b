"""Image tables built by hand for the tests of salsa_room_rirs (salsa_amd/csrc/room_rir.hip): what no physical room
gives the kernel's compaction -- waves in which all 64 lanes hit, chunks whose 256 slots are all used, a hit in the last lane of the
last wave alone -- and tables whose arithmetic is exact, so that the order of a tap's float32 sum can be read from its bits.

A table is the public float64 (7, n) array (rows: sign x, y, z, shift x, y, z, amplitude); image i lies at sign_i o s + shift_i.

  built_table(mask)    one source, a receiver off the axes, fs / c = 24000 / 343, made for 300 taps (block 0 of the kernel full, block 1
                       short).  A HIT image (mask true) lies at a random point whose delay is in [20, 270) with a random fraction -- so
                       its floor is at most 269 <= 256 + H - 2 and BLOCK 0 KEEPS EVERY HIT --, amplitude in (0.05, 1], random signs.  A
                       MISS lies 10^6 m away.  Image i draws the same numbers whatever the mask is.
  MASKS                the hit patterns: all hit at n around the wave (64), the chunk (256) and four chunks, and over n = 1024 a chunk of
                       misses, one lane per wave, whole waves, alternating lanes, the last index alone, none.
  big_first_table,     fs / c = 1, receiver and source at the origin, signs +1, whole shifts at whole distances: an image adds its
  random_exact_table   coefficient times exactly 1 to tap d and exactly 0 to its neighbours (see the section below).

Nothing here reads the code under test."""
import numpy as np

FS_OVER_C = 24000 / 343
LENGTH = 300
SEED = 20251
SOURCE = np.array([0.83, 1.71, 0.64])
RECEIVER = np.array([1.37, 0.91, 1.13])
# the omni receivers: the point the tables are built around, then three points a capsule's radius away from it
RECEIVERS = np.stack([RECEIVER, RECEIVER + [0.042, 0.0, 0.0], RECEIVER + [0.0, -0.042, 0.0], RECEIVER + [-0.024, 0.024, 0.024]])
MISS = 1e6                                                                     # metres


def source(t0=0.0, g=1.3):
    """(position, t0, g) as room_reference takes it"""
    return SOURCE.copy(), float(t0), float(g)


def source_row(src):
    """the (1, 5) row of salsa_room_rirs"""
    return np.array([[src[0][0], src[0][1], src[0][2], src[1], src[2]]], np.float64)


def built_table(mask, lo=20.0, hi=270.0, t0=0.0, seed=SEED):
    """mask (n) bool -> table (7, n): the hits with delays in [lo, hi) after t0, the misses 10^6 m away"""
    mask = np.asarray(mask, bool)
    n = len(mask)
    rng = np.random.RandomState(seed)
    delay = np.floor(rng.uniform(lo, hi, n)) + rng.uniform(0.0, 1.0, n)       # a whole part in [lo, hi - 1] and a random fraction
    u = rng.randn(3, n)
    u /= np.sqrt((u * u).sum(axis=0))
    sign = np.where(rng.rand(3, n) < 0.5, -1.0, 1.0)
    amp = 1.0 - 0.95 * rng.rand(n)                                             # (0.05, 1]
    p = RECEIVER[:, None] + ((delay + t0) / FS_OVER_C)[None] * u
    p = np.where(mask[None], p, np.array([MISS, 0.0, 0.0])[:, None])
    shift = p - sign * SOURCE[:, None]
    return np.ascontiguousarray(np.concatenate([sign, shift, amp[None]]), np.float64)


def _over_1024(keep):
    m = np.zeros(1024, bool)
    m[keep] = True
    return m


_I = np.arange(1024)
MASKS = {'all_%d' % n: np.ones(n, bool) for n in (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)}
MASKS.update({
    'chunk1_miss': _over_1024((_I < 256) | (_I >= 512)),
    'lane0': _over_1024(_I % 64 == 0),
    'lane63': _over_1024(_I % 64 == 63),
    'waves_0_2': _over_1024((_I // 64) % 2 == 0),                              # of every chunk: waves 0 and 2 full, 1 and 3 empty
    'alternating': _over_1024(_I % 2 == 0),
    'last_only': _over_1024(_I == 1023),
    'none': _over_1024(_I < 0),
})


def negative_delay_table(n=300, t0=40.0):
    """every delay in (-16, 4) with t0 > 0: supports cut at tap 0, floor(tau) < 0"""
    return built_table(np.ones(n, bool), lo=-16.0, hi=4.0, t0=t0, seed=SEED + 1)


# ---- exact arithmetic ------------------------------------------------------------------------------------------------------------
# fs / c = 1, receiver at the origin, source at the origin with signs +1: p = shift, d = |shift| a whole number for the shifts used,
# tau = d, the fraction 0, so an image adds its coefficient times exactly 1 to tap d and exactly +-0 to the other taps of its support.
EXACT_RECEIVER = np.zeros((1, 3))


def exact_source(g):
    return np.zeros(3), 0.0, float(g)


def exact_table(shifts, amps):
    shifts = np.asarray(shifts, np.float64).reshape(-1, 3)
    return np.ascontiguousarray(np.concatenate([np.ones((3, len(shifts))), shifts.T, np.asarray(amps, np.float64)[None]]), np.float64)


BIG_TAP, N_SMALL, SMALL = 40, 4096, 2.0 ** -25


def big_first_table():
    """amplitude 1, then 4096 duplicates of amplitude 2^-25 on the same tap (17 chunks of 256); with g = d = 40 a coefficient is its
    amplitude exactly.  Summed in this order tap 40 is 1.0f (2^-25 is a quarter ulp of 1), in the reversed order 2^-13 (exact) + 1."""
    return exact_table([(BIG_TAP, 0, 0)] * (1 + N_SMALL), [1.0] + [SMALL] * N_SMALL)


# whole-number triples by their length; the signed and permuted variants below put u's components on every channel with either sign
_TRIPLES = {29: [(12, 16, 21), (20, 21, 0), (0, 0, 29)], 33: [(4, 7, 32), (0, 33, 0)], 45: [(5, 20, 40), (27, 36, 0)],
            261: [(108, 144, 189), (180, 189, 0), (261, 0, 0)], 290: [(120, 160, 210), (200, 210, 0)]}


def random_exact_table(n=1000, seed=SEED + 2):
    """n images with random amplitudes on the taps 29, 33, 45 (block 0) and 261, 290 (block 1) -> (table, d (n): each image's tap)"""
    rng = np.random.RandomState(seed)
    taps = sorted(_TRIPLES)
    shifts, d = [], []
    for _ in range(n):
        t = taps[rng.randint(len(taps))]
        v = np.array(_TRIPLES[t][rng.randint(len(_TRIPLES[t]))], np.float64)[rng.permutation(3)] * np.where(rng.rand(3) < 0.5, -1.0, 1.0)
        assert float(v @ v) == float(t * t)
        shifts.append(v)
        d.append(t)
    amps = 1.0 - 0.95 * rng.rand(n)
    return exact_table(shifts, amps), np.array(d)


def sequential_float32(table, g, length):
    """what the exact geometry makes of a table: per FOA channel and tap the np.float32 sum, in table order, of float32(g A / d u_c),
    the coefficient formed in float64 as the definition says: (g A) / d, times (component / d).  -> (4, length) float32"""
    h = np.zeros((4, length), np.float32)
    for i in range(table.shape[1]):
        v, A = table[3:6, i], table[6, i]
        d = float(np.sqrt(v @ v))
        assert d == round(d) and 0 <= d < length
        coef = g * A / d
        for ch, gain in enumerate((coef, coef * (v[1] / d), coef * (v[2] / d), coef * (v[0] / d))):
            h[ch, int(d)] = np.float32(h[ch, int(d)] + np.float32(gain))
    return h
