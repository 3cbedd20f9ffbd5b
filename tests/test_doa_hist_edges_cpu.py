"""The DOA histogram off its default shapes, on the CPU: the built cases that tests/test_doa_hist_edges_gpu.py
runs on the kernel -- every grid step (so every instantiation of the kernel: 4, 10 and 28 cells a thread), windows with col0 > 0, of
4096 cells exactly, of less than one round and of less than one wave, 63 / 64 / 65 votes, K = 8 against eight and nine clusters,
thresholds off their defaults, lengths float32 cannot square -- each through the composed torch path against the float64 reference
of tests/doa_hist_reference.py under its margin condition, with no frame excluded; the bit identity of the first eleven cases' inputs;
and exact ties, which the margin condition keeps out of every built frame, by construction on the coordinate axes."""
import functools
import hashlib

import numpy as np
import pytest
import torch

import doa_hist_reference as ref
from salsa_amd import localize as lz
from test_doa_hist_cpu import CASES, as_dict, make_localizer

# sha256 over (shape, bytes) of the tensors build_features returned for CASES before it took a window, a frame count and a name list
BUILT_SHA256 = {
    ('foa', 7, 5): '3e52072a9ac5820920134b92fae1728e8c883d55ce46461d833020c9d736780a',
    ('foa', 7, 15): '024a0b64387380e3e825f114e9e5df26d0eeba6e825845720bed5ced243adcd9',
    ('mic', 7, 5): '948b1c319e24a10a7dd0724aa760ca9edf7805d13ebb93f4ea724ac669b79877',
    ('mic', 7, 15): 'fbf8adf50ad05686e296bb2a220fbd51a9aa62c9eb9c1774e4b4a63cef3054b1',
    ('mic', 10, 5): '56d407bd462f45c731e47b8354a65735c23237a9c3af36811e2148079ceb8c55',
    ('mic', 10, 15): '5ddb26e4b884d4cf52512340d564adecd14f065856906e827238580725da52e3',
}

WINDOW_4096 = dict(fmin_hz=500, fmax_hz=6520, frames_per_label=32)          # columns [10, 138) x 32 frames: the limit exactly
WINDOW_216 = dict(fmin_hz=200, fmax_hz=1500)                                # columns [4, 31) x 8 frames: col0 > 0, less than one round
NARROW = dict(kernel_deg=8.0, suppress_deg=22.0, min_score=3.0, norm_range=(0.9, 1.1))
WIDE = dict(kernel_deg=40.0, suppress_deg=100.0)
ALL_SUPPRESSED = dict(suppress_deg=180.0)                                   # cos_suppress = -1: the first peak suppresses every cell


def _case(group, fmt, K, step, names=ref.FRAME_NAMES, clips=3, label_frames=3, n_channels=7, window=None, seed=0, **kw):
    return dict(group=group, fmt=fmt, K=K, step=step, names=tuple(names), clips=clips, label_frames=label_frames, n_channels=n_channels,
                window=window, seed=seed, kw=dict(kw))


def _edge_cases():
    c = {}
    for fmt in ('foa', 'mic'):                                              # (a) every grid step the first list leaves out
        for step in (3, 6, 9, 10, 18, 30):
            c['a-%s-step%d' % (fmt, step)] = _case('a', fmt, 2 if step == 30 else 8, step, n_channels=10 if step == 9 else 7)
    for step in (3, 5, 30):                                                 # (b) the window's geometry
        c['b-foa-4096-step%d' % step] = _case('b', 'foa', 2 if step == 30 else 8, step, ('full4096', 'dense4096'), 1, 2, window=(10, 138),
                                              **WINDOW_4096)
    c['b-foa-216'] = _case('b', 'foa', 2, 5, window=(4, 31), **WINDOW_216)
    c['b-foa-p1'] = _case('b', 'foa', 2, 5, ref.FRAME_NAMES + ('n63', 'n64', 'n65'), 3, 7, window=(0, 191), frames_per_label=1)   # and (c)
    c['b-mic-p1'] = _case('b', 'mic', 2, 5, ('n0', 'n1', 'north', 'south', 'seam', 'above', 'below', 'full', 'dirty', 'n63', 'two', 'n256'),
                          3, 4, window=(0, 33), frames_per_label=1)
    for fmt in ('foa', 'mic'):
        for step in (3, 5, 15):                                             # (d) K = 8 against eight and nine clusters
            c['d-%s-step%d' % (fmt, step)] = _case('d', fmt, 8, step, ('eight', 'nine', 'nine', 'eight'), 2, 2)
        c['e-%s-narrow' % fmt] = _case('e', fmt, 4, 6, **NARROW)            # (e) thresholds off their defaults
        # suppress_deg = 100 on the 10-degree grid puts whole rings of cells ON the suppression cosine of a peak; with seed 0 the third
        # peak of 'full' (its background) is such a cell in both formats and the margin condition fails, with seed 5 none is
        c['e-%s-wide' % fmt] = _case('e', fmt, 4, 10, seed=5, **WIDE)
        c['e-%s-all-suppressed' % fmt] = _case('e', fmt, 4, 5, ('two', 'full', 'apart31'), 3, 1, **ALL_SUPPRESSED)
        c['f-%s-extreme' % fmt] = _case('f', fmt, 2, 5, ('extreme', 'dirty', 'extreme', 'n1'), 2, 2)       # (f) lengths float32 cannot square
    return c


EDGE_CASES = _edge_cases()
EDGE_IDS = sorted(EDGE_CASES)


@functools.lru_cache(maxsize=None)
def built_edge(name):
    """(localizer, [features], [reference]) of one edge case, computed once and shared with tests/test_doa_hist_edges_gpu.py"""
    c = EDGE_CASES[name]
    loc = make_localizer(c['fmt'], c['K'], c['step'], **c['kw'])
    if c['window'] is not None:
        assert (loc.col0, loc.col1) == c['window']
    xs = ref.build_features(loc, n_channels=c['n_channels'], names=c['names'], clips=c['clips'], label_frames=c['label_frames'],
                            seed=c['seed'])
    refs = [ref.reference(x, loc) for x in xs]
    for x in xs:
        assert x.shape[2] == c['label_frames'] * loc.frames_per_label + (loc.frames_per_label > 1)
        x.setflags(write=False)
    return loc, xs, refs


def named(name, refs, field):
    """{frame name: [the reference's `field` of each frame of that name]}"""
    out = {}
    flat = np.concatenate([r[field].reshape((-1,) + r[field].shape[2:]) for r in refs])
    for n, v in zip(EDGE_CASES[name]['names'], flat):
        out.setdefault(n, []).append(v)
    return out


def test_the_first_cases_inputs_did_not_move():
    """build_features took a window, a frame count and a name list: the tensors of the first eleven cases keep every bit, so the MEASURED
    table of tests/test_doa_hist_gpu.py keeps its meaning"""
    for fmt, n_channels, K, step in CASES:
        h = hashlib.sha256()
        for x in ref.build_features(make_localizer(fmt, K, step), n_channels=n_channels):
            assert x.shape == (3, n_channels, 25, 200) and x.dtype == np.float32
            h.update(str(x.shape).encode())
            h.update(x.tobytes())
        assert h.hexdigest() == BUILT_SHA256[fmt, n_channels, step], (fmt, n_channels, K, step)


@pytest.mark.parametrize('name', EDGE_IDS)
def test_torch_path_matches_the_float64_reference(name):
    loc, xs, refs = built_edge(name)
    for x, r in zip(xs, refs):
        ref.check_margins(r)                                # the condition: no frame of the built inputs is excluded
        got = as_dict(loc.localize(torch.from_numpy(x.copy()), spectrum=True))
        worst = ref.check_against(got, r, direction_tol=1e-5, what='torch %s' % name)
        print('TORCH %s %s' % (name, worst))
        assert np.all(got['cell'][got['cell'] < 0] == -1)


def test_edge_frames_are_what_they_are_named():
    """the vote counts, peaks and exits the edge list promises, by the reference alone"""
    for step in (3, 5, 30):
        name = 'b-foa-4096-step%d' % step
        loc, xs, refs = built_edge(name)
        assert loc.frames_per_label * (loc.col1 - loc.col0) == lz.MAX_VOTES
        assert named(name, refs, 'n_votes') == {'full4096': [4096], 'dense4096': [4096]}
        if step < 30:                                       # the refinement sums (nearly) every vote of the larger cluster; at 30 degrees
            assert named(name, refs, 'n_in')['dense4096'][0][0] >= 2490        # the winning cell lies too far from the cluster's centre
    for name, cells in (('b-foa-216', 216), ('b-foa-p1', 191), ('b-mic-p1', 33)):
        loc, xs, refs = built_edge(name)
        assert loc.frames_per_label * (loc.col1 - loc.col0) == cells
        assert named(name, refs, 'n_votes')['full'][0] == cells
    votes = named('b-foa-p1', built_edge('b-foa-p1')[2], 'n_votes')
    assert (votes['n63'], votes['n64'], votes['n65']) == ([63], [64], [65])
    for fmt in ('foa', 'mic'):
        for step in (3, 5, 15):
            name = 'd-%s-step%d' % (fmt, step)
            loc, xs, refs = built_edge(name)
            assert all(c == 8 for c in named(name, refs, 'count')['eight'] + named(name, refs, 'count')['nine'])
            for cells in named(name, refs, 'cell')['nine']:                 # the eight strongest of nine: the 20-vote cluster is left out
                az, el = loc.azimuth[cells], loc.elevation[cells]
                weakest = ref.off_grid(loc, *ref.CLUSTER_CENTRES[0])
                assert ref.angle_deg(ref.unit(az, el), ref.unit(*weakest)).min() > 30.0
        if fmt == 'foa':
            assert all(c == 8 for c in named('a-foa-step3', built_edge('a-foa-step3')[2], 'count')['full'])
        name = 'e-%s-all-suppressed' % fmt
        loc, xs, refs = built_edge(name)
        assert loc.cos_suppress == -1.0 and loc.max_sources == 4
        assert all(c <= 1 for cs in named(name, refs, 'count').values() for c in cs)
        assert named(name, refs, 'count')['two'] == [1] and named(name, refs, 'count')['full'] == [1]    # the exit after the first peak
        name = 'f-%s-extreme' % fmt
        loc, xs, refs = built_edge(name)
        assert named(name, refs, 'n_votes')['extreme'] == [40, 40] and named(name, refs, 'count')['extreme'] == [1, 1]
        # the narrow norm range rejects some of the built lengths (0.8 .. 1.25)
        name = 'e-%s-narrow' % fmt
        loc, xs, refs = built_edge(name)
        default = [ref.reference(x, make_localizer(fmt, 4, 6)) for x in xs]
        narrow, wide = named(name, refs, 'n_votes'), named(name, default, 'n_votes')
        for frame in ('n255', 'full', 'two', 'seam'):
            assert narrow[frame][0] < wide[frame][0], (frame, narrow[frame], wide[frame])


# ---------------------------------------------------------------------------------------------------------------- exact ties
# (x, y, z) of the six axes.  As channels (4, 5, 6) = (y, z, x) a vote is a single +-1 and two +0.0: its length is exactly 1, its dot with
# the axis' own cell exactly 1.0f in any evaluation order (the table holds +-1 there beside 6.1e-17 or 0), the term (1 - c0) inv is
# exactly 1.0f for the default cap, and every other cell within the cap scores less: equal vote counts give equal bits.
AXES = {'+x': (1, 0, 0), '-x': (-1, 0, 0), '+y': (0, 1, 0), '-y': (0, -1, 0), '+z': (0, 0, 1), '-z': (0, 0, -1)}
AXIS_CELL = {'+x': (0, 0), '-x': (-180, 0), '+y': (90, 0), '-y': (-90, 0), '+z': (0, 90), '-z': (0, -90)}
# frame -> the axes in VOTE order (round robin, ten votes each; not the cells' order) and the axes in the order the peaks must come
TIE_FRAMES = (('poles', ('+z', '-z'), ('-z', '+z')),
              ('equator', ('+y', '+x', '-y', '-x'), ('-x', '-y', '+x', '+y')),
              ('six', ('+z', '+y', '+x', '-y', '-x', '-z'), ('-z', '-x', '-y', '+x', '+y', '+z')))
# The kernel's wave of each tied cell, in peak order: thread = cell mod 256, wave = thread / 64.  Tied cells in ONE wave meet in the
# 64-lane butterfly, tied cells in DIFFERENT waves in the merge of the four waves' winners; a frame can hold both.
#   step 3  (G = 7082): poles 0 and 7081 -> waves 0, 2: the merge.  Equator 3481, 3511, 3541, 3571 -> waves 2, 2, 3, 3: both.
#   step 5  (G = 2522): poles 0 and 2521 -> waves 0, 3: the merge.  Equator 1225, 1243, 1261, 1279 -> wave 3, all four: the butterfly.
#   step 30 (G = 62):   every cell in wave 0: the butterfly alone; waves 1 to 3 own no cell and bring g = INT_MAX to the merge.
TIE_WAVES = {3: {'poles': (0, 2), 'equator': (2, 2, 3, 3), 'six': (0, 2, 2, 3, 3, 2)},
             5: {'poles': (0, 3), 'equator': (3, 3, 3, 3), 'six': (0, 3, 3, 3, 3, 3)},
             30: {'poles': (0, 0), 'equator': (0, 0, 0, 0), 'six': (0, 0, 0, 0, 0, 0)}}
# Two tied cells of ONE thread (indices 256 k apart: the per-thread scan's "the lowest index of a tie stays") exist at steps 3 and 5:
# (azimuth 0, elevation -e) and (0, +e) are (2 e / s)(360 / s) cells apart, 15 x 256 at s = 3, e = 48 and 9 x 256 at s = 5, e = 80.
# Two votes each (the cells' own table vectors, mirror images in z, so every operation on one is the mirror of that on the other, and
# t + t is exact whatever the order of summation), hence min_score 1.5 for this frame alone.
THREAD_TIE_ELEVATION = {3: 48, 5: 80}


def cell_of(loc, az, el):
    at = np.nonzero((loc.azimuth == az) & (loc.elevation == el))[0]
    assert len(at) == 1
    return int(at[0])


def _tie_features(loc, frames):
    """float32 (1, 7, 8 len(frames), 200): frame f's votes (x, y, z), in order, at every 7th cell of its window from the 5th on (two
    rounds of the compaction for 60 votes); every other value +0.0"""
    P, ncol = loc.frames_per_label, loc.col1 - loc.col0
    x = np.zeros((1, 7, P * len(frames), 200), np.float32)
    for f, votes in enumerate(frames):
        for i, d in enumerate(np.asarray(votes, np.float32)):
            t, col = divmod(5 + 7 * i, ncol)
            x[0, 4:7, f * P + t, loc.col0 + col] = d[[1, 2, 0]]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def tie_case(step):
    """(localizer, features, [(frame name, the tied cells in peak order, their directions float32 (n, 3))])"""
    loc = make_localizer('foa', 8, step)
    frames, expect = [], []
    for name, vote_order, peak_order in TIE_FRAMES:
        frames.append([AXES[vote_order[i % len(vote_order)]] for i in range(10 * len(vote_order))])
        cells = [cell_of(loc, *AXIS_CELL[a]) for a in peak_order]
        assert cells == sorted(cells) and tuple((g % 256) // 64 for g in cells) == TIE_WAVES[step][name]
        expect.append((name, cells, np.array([AXES[a] for a in peak_order], np.float32)))
    return loc, _tie_features(loc, frames), expect


@functools.lru_cache(maxsize=None)
def thread_tie_case(step):
    """the same for the one frame whose two tied cells belong to one thread of the kernel; directions: the cells' table vectors"""
    loc = make_localizer('foa', 8, step, min_score=1.5)
    e = THREAD_TIE_ELEVATION[step]
    lo, hi = cell_of(loc, 0, -e), cell_of(loc, 0, e)
    assert hi > lo and (hi - lo) % 256 == 0
    assert np.array_equal(loc.grid[lo] * np.float32([1, 1, -1]), loc.grid[hi])
    return loc, _tie_features(loc, [[loc.grid[hi], loc.grid[lo], loc.grid[hi], loc.grid[lo]]]), [('thread', [lo, hi], None)]


def check_ties(got, expect, what):
    """got: arrays shaped as DoaResult's for ONE clip.  Per frame: the count, the cells in the promised order, equal bits in the tied
    scores, the directions (the axes exactly; for the 'thread' frame mirror images of each other in z), unused slots"""
    for f, (name, cells, axes) in enumerate(expect):
        n = len(cells)
        assert got['count'][0, f] == n, '%s %s: count %d' % (what, name, got['count'][0, f])
        assert list(got['cell'][0, f, :n]) == cells and np.all(got['cell'][0, f, n:] == -1), '%s %s: cells %s' % (what, name, got['cell'][0, f])
        score, d = np.asarray(got['score'][0, f]), np.asarray(got['direction'][0, f])
        bits = score[:n].view(np.uint32 if score.dtype == np.float32 else np.uint64)
        assert np.all(bits == bits[0]) and score[0] >= 1.5, '%s %s: the tied scores differ: %s' % (what, name, score[:n])
        assert np.all(score[n:] == 0) and np.all(d[n:] == 0)
        if axes is not None:
            assert got['n_votes'][0, f] == 10 * n
            assert score[0] == 10.0 or score.dtype != np.float32            # ((1 - c0) inv is 1.0f exactly; in float64 it is 1 + 4.9e-9)
            assert np.array_equal(d[:n], axes), '%s %s: directions %s' % (what, name, d[:n])
        else:
            assert got['n_votes'][0, f] == 4
            assert np.array_equal(d[0] * np.array([1, 1, -1], d.dtype), d[1]), '%s %s: directions %s' % (what, name, d[:n])
    return True


def _frame_votes(loc, x, f):
    P = loc.frames_per_label
    return x[0, 4:7, f * P:(f + 1) * P, loc.col0:loc.col1].transpose(1, 2, 0).reshape(-1, 3)


TIE_BUILDERS = [(tie_case, 3), (tie_case, 5), (tie_case, 30), (thread_tie_case, 3), (thread_tie_case, 5)]
TIE_IDS = ['%s-step%d' % (b.__wrapped__.__name__, s) for b, s in TIE_BUILDERS]


@pytest.mark.parametrize('builder,step', TIE_BUILDERS, ids=TIE_IDS)
def test_exact_ties_go_to_the_lowest_index(builder, step):
    """float32 in the kernel's stated order (the proof that the scores tie, bit for bit, and that no other cell reaches them), the
    composed torch path and the float64 reference (its margin failures are ignored here: a tie has no margin)"""
    loc, x, expect = builder(step)
    stated = [ref.kernel_order_float32(_frame_votes(loc, x, f), loc) for f in range(len(expect))]
    for s, (name, cells, axes) in zip(stated, expect):
        others = np.ones(loc.n_cells, bool)
        others[cells] = False
        assert np.all(s['spectrum'][cells].view(np.uint32) == s['spectrum'][cells[0]].view(np.uint32))
        assert s['spectrum'][others].max() < s['spectrum'][cells[0]], name
        if axes is not None:
            assert np.array_equal(np.abs(loc.grid[cells]).max(axis=1), np.ones(len(cells), np.float32))     # the table holds +-1 there
    as_result = {k: np.stack([s[k] for s in stated])[None] for k in ('count', 'n_votes', 'cell', 'score', 'direction')}
    check_ties(as_result, expect, 'float32 as stated')
    got = as_dict(loc.localize(torch.from_numpy(x.copy()), spectrum=True))
    check_ties(got, expect, 'torch')
    for s, f in zip(stated, range(len(expect))):               # nothing in these frames rounds differently in the torch path
        assert np.array_equal(got['score'][0, f].view(np.uint32), s['score'].view(np.uint32))
    r = ref.reference(x, loc)
    assert r['failures']                                        # ties ARE margin failures
    check_ties(r, expect, 'float64 reference')
