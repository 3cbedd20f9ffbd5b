"""CPU half of the noise-floor tracker's bit-for-bit check (tests/tracker_reference.py; the GPU half is test_tracker_gpu.py).

The float64 restatement is tied to the reference through the sig_mask arrays of fixtures g1 / g2 and to the C oracle on every
case of the table; every case gives one mask whether the power is formed as |X0|^2 or as re^2 + im^2; each aimed family is shown
from the restatement's trace to reach the branch it is built for; and each deliberate change of the restatement is exposed by
the cases the table names, so a kernel with that fault cannot pass the GPU half.  Fixture g27 holds the reference's own masks of the small aimed blocks."""
import time

import numpy as np
import pytest

import tracker_reference as tr
from conftest import load_golden
from salsa_amd.synth import sha256_of, synth_stft_block

CLOCK = {}


@pytest.fixture(scope='module', autouse=True)
def _clock():
    """started by this module's first test (collection of the other test files is not counted)"""
    CLOCK['t0'] = time.time()
    yield


def _oracle_sig(oracle, X):
    return np.stack([oracle.extract_normalized_eigenvector(x, 0.0, 3, True, 'foa', fs=24000, n_fft=512, lower_bin=1,
                                                           return_aux=True)[1]['sig'] for x in X])


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_restatement_equals_reference_golden_g1(seed):
    meta, a = load_golden('g1_eigvec_s%d' % seed)
    X = synth_stft_block(seed, meta['n_bins'], meta['n_frames'], kind=meta['kind'])
    assert sha256_of(X) == meta['sha']
    for power in ('hypot', 'sumsq'):
        assert np.array_equal(tr.tracker_mask(X, power=power), a['sig_mask'])


def test_restatement_equals_reference_golden_g2():
    meta, a = load_golden('g2_adversarial')
    assert len(meta['cases']) == 6
    for case in meta['cases']:
        for power in ('hypot', 'sumsq'):
            assert np.array_equal(tr.tracker_mask(a['X_' + case], power=power), a[case + '_sig_mask']), (case, power)


def test_case_table_covers_the_shapes():
    frames = {c[4] for c in tr.CASES}
    bins = {c[3] for c in tr.CASES}
    assert frames >= {1, 2, 3, 4, 5, 6, 63, 64, 65, 127, 128, 129, 191, 192, 193, 4801}
    assert bins >= {1, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 191, 200}
    assert {c[2] for c in tr.CASES} >= {1, 3, 32}
    assert len(set(tr.CASE_NAMES)) == len(tr.CASES)
    assert set(tr.SOLVER_SUBSET) | set(tr.FORMAT_SUBSET) | {tr.ALL_SILENT} <= set(tr.CASE_NAMES)


def test_every_case_against_oracle_both_powers_and_density(oracle):
    """restatement == oracle sig, 'hypot' == 'sumsq', density strictly inside (0, 1) per case and inside [10 %, 90 %] overall"""
    ones = total = 0
    for name in tr.CASE_NAMES:
        t0 = time.time()
        X, _ = tr.build_case(name)
        m = tr.tracker_mask(X)
        assert np.array_equal(m, tr.tracker_mask(X, power='sumsq')), '%s: |X0|^2 and re^2 + im^2 give different masks (rebuild with another seed)' % name
        sig = _oracle_sig(oracle, X)
        assert np.array_equal(m, sig), '%s: %s' % (name, tr.describe_first_difference(sig, m, X))
        clips = {sha256_of(x) for x in X} | {sha256_of(x) for x in m}           # every clip of a batch is its own track, with its own mask
        assert len(clips) == 2 * X.shape[0], '%s: a batch holds the same clip twice' % name
        print('%-20s %s density %.4f (%d bits) %.1f s' % (name, X.shape[:3], m.mean(), m.size, time.time() - t0))
        if name == tr.ALL_SILENT:
            assert not m.any() and not X[..., 0].any()
        else:
            assert 0 < m.sum() < m.size, name
        ones, total = ones + int(m.sum()), total + m.size
    print('whole table: %d of %d bits set (%.2f %%)' % (ones, total, 100.0 * ones / total))
    assert 0.10 <= ones / total <= 0.90


def test_real_only_families_have_real_channel_0():
    for name in tr.CASE_NAMES:
        if tr.case(name)[1] not in ('random',):
            X, _ = tr.build_case(name)
            assert not X[..., 0].imag.any(), name


def test_clamp_cases_reach_the_clamp_on_the_chunk_boundaries():
    seen = set()
    for name in ('clamp_33x129', 'clamp_65x4801'):
        X, info = tr.build_case(name)
        _, t = tr.tracker_mask(X[0], trace=True)
        start_silent = [b for b in range(X.shape[1]) if not X[0, b, :5, 0].any()]
        assert len(start_silent) >= X.shape[1] - 3
        assert t['floor_before'][start_silent, 0].max() == 0.0            # the floor starts at exactly 0: the 0 > 0 tie
        assert not t['above'][start_silent, 0].any()
        for b, f in info[0]['clamp_frames']:
            assert t['clamped'][b, f] and t['floor'][b, f] == 1e-6 and t['floor_before'][b, f] == 1e-6, (name, b, f)
            seen.add(f)
    assert seen == {63, 64, 127, 128, 4799, 4800}
    X, info = tr.build_case('clamp_65x4801')
    _, t = tr.tracker_mask(X[0], trace=True)
    lv = np.abs(X[0, :, :, 0].real)
    for v in (1e-6, 1.5e-6, 4e-6):                                        # constant levels at, just below and just above
        f32 = np.float32(v)
        for w in (np.nextafter(f32, np.float32(0)), f32, np.nextafter(f32, np.float32(1))):
            assert (lv == w).any(), (v, w)
    assert t['floor'][0, 1999] > 0.9 and t['floor'][0, 2600] > 1e-6 and t['floor'][0, 4000:].max() == 1e-6  # bin 0: from a loud floor onto the clamp
    assert info[0]['first_clamp'] == [(3, 703), (4, 704)]                 # a floor that decays from 0.4 and MEETS the clamp at a boundary
    for b, f in info[0]['first_clamp']:
        assert t['floor_before'][b, 0] > 0.3 and not t['clamped'][b, :f].any() and t['clamped'][b, f:].all(), (b, f)
        assert t['floor_before'][b, f] > 1e-6 and t['floor'][b, f] == 1e-6


def test_slow_rise_lands_on_the_four_offsets_around_a_boundary():
    X, info = tr.build_case('slowrise_33x193')
    _, t = tr.tracker_mask(X[0], trace=True)
    offsets = set()
    for b, s, first in info[0]['slow']:
        assert not t['above'][b, s - 1] and t['above'][b, s:first + 1].all(), (b, s)
        assert not t['slow'][b, s:first].any() and t['slow'][b, first], (b, s, first)
        if (b // 4) % 3 == 0:
            offsets.add((first + 1) % tr.TR_CH)
    assert offsets == {0, 1, 2, 3}                                         # frames 64 j - 1, 64 j, 64 j + 1, 64 j + 2
    assert {first // tr.TR_CH for _, _, first in info[0]['slow']} >= {0, 1, 2}
    dips = set()
    for b, d in info[0]['dips']:
        assert t['above'][b, d - 3:d].all() and not t['above'][b, d] and t['above'][b, d + 1], (b, d)
        assert t['countdown'][b, d] == 3 and t['countdown'][b, d - 1] < 3
        dips.add((d + 1) % tr.TR_CH)
    assert dips == {0, 1}                                                  # right before and right after a boundary


def test_knife_edges_differ_in_the_targeted_bit():
    name = [n for n in tr.CASE_NAMES if tr.case(n)[1] == 'knife'][0]
    X, info = tr.build_case(name)
    a = X[0, :, :, 0].real
    m, t = tr.tracker_mask(X[0], trace=True)
    m_ge = tr.tracker_mask(X[0], mutate='ge')
    kinds = set()
    for kind, f, bins in info[0]['targets']:
        kinds.add((kind, f // tr.TR_CH))
        if kind == 'tie':
            b, = bins
            assert t['mag'][b, f] == t['floor_before'][b, f] and not t['above'][b, f]      # an exact tie, decided by strictness
            d = np.flatnonzero(m[b] != m_ge[b])
            assert d.size and d[0] >= f
            continue
        lo, hi = bins
        d = np.flatnonzero(a[lo] != a[hi])
        assert d.tolist() == [f] and a[hi, f] == np.nextafter(a[lo, f], np.float32(np.inf))    # adjacent float32 amplitudes
        d = np.flatnonzero(m[lo] != m[hi])
        if kind == 'sig':
            assert d.tolist() == [f] and not m[lo, f] and m[hi, f]
        else:
            assert not t['above'][lo, f] and t['above'][hi, f] and np.array_equal(t['above'][lo, :f], t['above'][hi, :f])
            assert d.size and d[0] >= f                                     # the masks part from that frame on
    assert kinds >= {(k, c) for k in ('floor', 'sig') for c in (0, 1, 2, 3)}    # first chunk, after boundaries, ragged tail


def test_wrap_cases_depend_on_the_wrapped_frames():
    for name in tr.CASE_NAMES:
        if tr.case(name)[1] == 'wrap':
            X, _ = tr.build_case(name)
            m, t = tr.tracker_mask(X, trace=True)
            _, t_nowrap = tr.tracker_mask(X, trace=True, mutate='nowrap')
            assert (t['floor_before'][..., 0] != t_nowrap['floor_before'][..., 0]).all(), name      # the initial floor
            assert not np.array_equal(m[..., :2], tr.tracker_mask(X, mutate='nowrap')[..., :2]), name


def test_each_deliberate_fault_is_caught_by_the_cases_the_table_names():
    caught = {q: [] for q in tr.MUTANTS}
    for name in tr.CASE_NAMES:
        claims = tr.case(name)[6]
        if not claims:
            continue
        X, _ = tr.build_case(name)
        m = tr.tracker_mask(X)
        for q in claims:
            n = int((tr.tracker_mask(X, mutate=q) != m).sum())
            assert n > 0, '%s no longer exposes %s' % (name, q)
            caught[q].append((name, n))
    print('deliberate fault -> (case, differing bits): %s' % caught)
    assert all(caught.values()), caught


def test_restatement_equals_reference_golden_g27():
    """the reference's own sig masks of the small aimed blocks (tools/make_golden.py g27, made the way g1's sig_mask is)"""
    meta, a = load_golden('g27_tracker')
    assert set(meta['cases']) == set(tr.GOLDEN_CASES)
    for name in meta['cases']:
        X, _ = tr.build_case(name)
        assert sha256_of(X) == meta['sha'][name], 'the track builders drifted from fixture g27 (%s)' % name
        want = np.unpackbits(a[name])[:X[..., 0].size].reshape(X.shape[:3]).astype(bool)
        for power in ('hypot', 'sumsq'):
            assert np.array_equal(tr.tracker_mask(X, power=power), want), (name, power)


def test_zz_report_time():
    print('tracker CPU tests: %.1f s added to the suite' % (time.time() - CLOCK['t0']))
