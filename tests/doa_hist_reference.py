"""The float64 reference of the DOA histogram (salsa_amd/localize.py, include/salsa_hip.h: salsa_doa_hist), its error bounds with their
rounding counts, the conditions under which decisions are compared exactly, the built vote sets of tests/test_doa_hist_cpu.py,
tests/test_doa_hist_gpu.py and the two tests/test_doa_hist_edges_*.py, and a float32 evaluation in the stated operation order for the
frames built to tie (kernel_order_float32).  numpy only; the constants (grid table, c0, inv, cos_suppress, matrix, norm range) are the float32 values of
the DoaHistogram under test, read as float64, so reference and code disagree by rounding alone.

Bounds (u = 2^-24, float32 unit roundoff; every product below carries a factor 1.01 for the second-order terms):
  vote       FOA: the inputs are exact.  length: three roundings in the sum of squares (1.5 u on n^2, 0.75 u on n), the root 0.5 u; the
             division 0.5 u: each component of u is within E_U = 2 u.
             MIC: a component of M v has three roundings on magnitudes <= A_i = sum_j |M_ij| |v_j|: 1.5 u A_i, i.e. 1.5 kappa u of
             the length, kappa = max_i A_i / |M v| (computed per vote, the frame's largest is used); the length inherits sqrt(3) of
             it: E_U = 2 + 1.5 (1 + sqrt 3) kappa.
  dot        three products and two sums on magnitudes <= 1: 2.5 u, plus the vote's error on |U_x| + |U_y| + |U_z| <= sqrt 3:
             EPS_DOT = (2.5 + sqrt(3) E_U) u.  (Any order of the three products, fused or not, stays inside: the torch path's matmul.)
  term       (dot - c0) inv: the subtraction u / 2 of <= 1 - c0, the product u / 2 of <= 1, the dot's error times inv:
             EPS_TERM = inv EPS_DOT + u.
  score[g]   n_g terms can be non-zero in either arithmetic: the votes with dot > c0 - EPS_DOT.  Adding a zero is exact; each other
             addition rounds a partial sum <= S_g: BOUND_g = n_g EPS_TERM + n_g (u / 2) S_g.  This holds for any order of summation.
  direction  m = the sum of n_in votes inside the cap, so m . U* >= n_in c0.  Per component: the votes' errors n_in E_U u, the
             additions (n_in - 1) (u / 2) n_in; as a 2-norm sqrt 3 of that, relative to |m|; the normalisation 2 u:
             DIR_BOUND = (sqrt(3) ((n_in - 1) / 2 + E_U) / c0 + 2) u.  (A worst case: the sums' errors grow like sqrt(n_in) in practice.)
Decisions (count, cell, n_votes) are compared exactly on frames where the reference's every decision has a margin (check_margins):
  - no vote's length within 4e-6 (relative; MIC 4e-6 kappa) of a norm limit;
  - every winner beats every other cell that is, or within 1e-6 of the suppression cosine might be, unsuppressed by more than twice
    the larger of the two bounds, and no winner is itself such a doubtful cell;
  - no winner's score, and no first loser's, within its bound of min_score;
  - no vote within 1e-6 of a winner's cap edge (it would enter or leave the refinement sum).
The built sets keep these by placing cluster centres off the grid's symmetry points: cell centre + (0.3 s, 0.2 s).

Measured with this reference on the CPU conventions test's inputs (2-s plane waves, oracle features, worst over 20 label frames and the
three directions (30, 10), (-120, -40), (170, 60)): MEASURED_SINGLE below, beside the bounds.  MIC on the rigid sphere: 3.76, 2.12 and
3.30 degrees for the three directions, one peak in 20 of 20 frames each; its bound is max(2, 2 x 3.76) = 7.52 degrees."""
import numpy as np

U = 2.0 ** -24
SLACK = 1.01
AMBIG = 1e-6

# worst angular error in degrees of the float64 reference, one peak in 20 of 20 label frames in every case
MEASURED_SINGLE = {'foa': 0.09, 'mic_open': 0.46, 'mic_rigid': 3.76, 'lite': 0.29}
SINGLE_RIGID_BOUND_DEG = max(2.0, 2.0 * MEASURED_SINGLE['mic_rigid'])                       # 7.52: the larger of 2 and twice the measured value
SINGLE_BOUND_DEG = {'foa': 2.0, 'mic_open': 2.0, 'lite': 2.0}                                # the issue's; mic_rigid: max(2, 2 x measured)


def unit(az_deg, el_deg):
    az, el = np.deg2rad(np.asarray(az_deg, np.float64)), np.deg2rad(np.asarray(el_deg, np.float64))
    return np.stack([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)], axis=-1)


def angle_deg(a, b):
    return np.rad2deg(np.arccos(np.clip(np.sum(np.asarray(a, np.float64) * np.asarray(b, np.float64), axis=-1), -1.0, 1.0)))


class FrameRef:
    pass


def frame_reference(v, loc):
    """One label frame.  v float32 (n_cells, 3): channels 4, 5, 6 of its cells in vote order.  -> FrameRef with count, n_votes, cell
    (K,), score (K,), direction (K, 3), spectrum (G,), bound (G,) the score bounds, dir_bound (K,), and .margin_failures, a list of
    strings (empty: every decision has its margin)."""
    K, G = loc.max_sources, loc.n_cells
    Ug = loc.grid.astype(np.float64)
    c0, inv, cs = float(loc.c0), float(loc.inv), float(loc.cos_suppress)
    v = np.asarray(v, np.float32).astype(np.float64).reshape(-1, 3)
    with np.errstate(invalid='ignore', over='ignore'):
        ok = np.isfinite(v).all(axis=1) & (v != 0).any(axis=1)
        vz = np.where(ok[:, None], v, 0.0)
        if loc.matrix is not None:
            M = loc.matrix.astype(np.float64)
            u = vz @ M.T
            absum = np.abs(vz) @ np.abs(M).T
        else:
            u = vz[:, [2, 0, 1]]
            absum = None
        length = np.sqrt((u * u).sum(axis=1))
    fails = []
    kappa = 0.0
    if absum is not None and ok.any():
        with np.errstate(invalid='ignore', divide='ignore'):
            kap = np.where(ok & (length > 0), absum.max(axis=1) / length, 0.0)
        kappa = float(kap[np.isfinite(kap)].max()) if np.isfinite(kap).any() else 0.0
    e_u = 2.0 + (1.5 * (1.0 + np.sqrt(3.0)) * kappa if absum is not None else 0.0)
    rel = 4e-6 * max(1.0, kappa)
    for lim in (loc.norm_lo, loc.norm_hi):
        if np.any(ok & (np.abs(length - lim) <= rel * lim)):
            fails.append('a vote length within %.1e of the limit %g' % (rel, lim))
    ok = ok & (length >= loc.norm_lo) & (length <= loc.norm_hi)
    u = u[ok] / length[ok][:, None]
    r = FrameRef()
    r.n_votes, r.e_u = int(ok.sum()), e_u
    eps_dot = (2.5 + np.sqrt(3.0) * e_u) * U * SLACK
    eps_term = (inv * eps_dot + U) * SLACK
    dots = u @ Ug.T                                                                             # (n, G)
    r.spectrum = np.maximum(0.0, (dots - c0) * inv).sum(axis=0)
    n_near = (dots > c0 - eps_dot).sum(axis=0)
    r.bound = (n_near * eps_term + n_near * (U / 2) * r.spectrum) * SLACK
    r.cell, r.score, r.direction = np.full(K, -1, np.int64), np.zeros(K), np.zeros((K, 3))
    r.dir_bound, r.n_in = np.zeros(K), np.zeros(K, np.int64)
    free, doubt, surely = np.ones(G, bool), np.zeros(G, bool), np.zeros(G, bool)       # surely: suppressed with a margin by some peak
    r.count = 0
    for k in range(K):
        if not free.any():
            break
        s = np.where(free, r.spectrum, -1.0)
        g = int(np.argmax(s))                                                                   # the first of the largest
        if s[g] < loc.min_score:
            if s[g] + r.bound[g] >= loc.min_score:
                fails.append('peak %d: the first loser %.6f is within %.2e of min_score' % (k, s[g], r.bound[g]))
            rivals = np.where(doubt & ~free & ~surely, r.spectrum + r.bound, -1.0)
            if rivals.max() >= loc.min_score:
                fails.append('peak %d: a doubtfully suppressed cell could still pass min_score' % k)
            break
        if s[g] - r.bound[g] <= loc.min_score:
            fails.append('peak %d: the winner %.6f is within %.2e of min_score' % (k, s[g], r.bound[g]))
        if doubt[g]:
            fails.append('peak %d: the winner is a doubtfully suppressed cell' % k)
        others = np.where(free | (doubt & ~surely), r.spectrum, -1.0)
        others[g] = -1.0
        j = int(np.argmax(others))
        if others[j] >= 0 and s[g] - others[j] <= 2.0 * max(r.bound[g], r.bound[j]):
            fails.append('peak %d: winner %.6f (cell %d) leads cell %d by %.2e, twice the bound is %.2e'
                         % (k, s[g], g, j, s[g] - others[j], 2.0 * max(r.bound[g], r.bound[j])))
        d = dots[:, g]
        if np.any(np.abs(d - c0) <= AMBIG):
            fails.append('peak %d: a vote within %.0e of the cap edge' % (k, AMBIG))
        inside = d >= c0
        m = u[inside].sum(axis=0)
        r.cell[k], r.score[k], r.direction[k] = g, s[g], m / np.sqrt(m @ m)
        r.n_in[k] = int(inside.sum())
        r.dir_bound[k] = (np.sqrt(3.0) * ((r.n_in[k] - 1) / 2.0 + e_u) / c0 + 2.0) * U * SLACK
        r.count += 1
        gg = Ug @ Ug[g]
        doubt |= np.abs(gg - cs) <= AMBIG
        surely |= gg > cs + AMBIG
        free &= ~(gg >= cs)
    r.margin_failures = fails
    return r


def reference(features, loc):
    """features float32 (B, C, T, F) numpy -> dict of arrays shaped as DoaResult's, plus bound (B, Fl, G), dir_bound (B, Fl, K), n_in and
    failures [(b, f, text)]"""
    x = np.asarray(features)
    B, _, T, _ = x.shape
    P, K, G = loc.frames_per_label, loc.max_sources, loc.n_cells
    Fl = T // P
    out = dict(count=np.zeros((B, Fl), np.int64), n_votes=np.zeros((B, Fl), np.int64), cell=np.zeros((B, Fl, K), np.int64),
               score=np.zeros((B, Fl, K)), direction=np.zeros((B, Fl, K, 3)), spectrum=np.zeros((B, Fl, G)), bound=np.zeros((B, Fl, G)),
               dir_bound=np.zeros((B, Fl, K)), n_in=np.zeros((B, Fl, K), np.int64), failures=[])
    for b in range(B):
        for f in range(Fl):
            v = x[b, 4:7, f * P:(f + 1) * P, loc.col0:loc.col1].transpose(1, 2, 0).reshape(-1, 3)
            r = frame_reference(v, loc)
            for name in ('count', 'n_votes', 'cell', 'score', 'direction', 'spectrum', 'bound', 'dir_bound', 'n_in'):
                out[name][b, f] = getattr(r, name)
            out['failures'] += [(b, f, t) for t in r.margin_failures]
    return out


def check_margins(ref):
    """the condition of the exact comparisons: every frame of the built inputs has its margins, so no frame is excluded"""
    assert not ref['failures'], 'frames without a decision margin: %s' % (ref['failures'][:5],)


def check_against(got, ref, direction_tol=None, what=''):
    """got: arrays shaped as DoaResult's (numpy).  Decisions exact, scores within the cells' bounds, directions within dir_bound (or
    direction_tol where given), unused slots exactly -1 / +0.0, the spectrum (if present) within the bounds.  -> worst ratios."""
    worst = {}
    for name in ('count', 'n_votes', 'cell'):
        assert np.array_equal(np.asarray(got[name], np.int64), ref[name]), '%s: %s differs' % (what, name)
    used = ref['cell'] >= 0
    sb = np.take_along_axis(ref['bound'], np.maximum(ref['cell'], 0), axis=2)
    err = np.abs(np.asarray(got['score'], np.float64) - ref['score'])
    assert np.all(err[used] <= sb[used]), '%s: score error %.3e above its bound' % (what, (err[used] / sb[used]).max())
    worst['score'] = float((err[used] / sb[used]).max()) if used.any() else 0.0
    derr = np.abs(np.asarray(got['direction'], np.float64) - ref['direction']).max(axis=-1)
    tol = ref['dir_bound'] if direction_tol is None else np.full_like(ref['dir_bound'], direction_tol)
    assert np.all(derr[used] <= tol[used]), '%s: direction error %.3e, %.2f of its bound' % (what, derr[used].max(), (derr[used] / tol[used]).max())
    worst['direction'] = float((derr[used] / tol[used]).max()) if used.any() else 0.0
    sc, dr = np.asarray(got['score']), np.asarray(got['direction'])
    assert np.all(sc[~used].view(np.uint32) == 0) and np.all(dr[~used].view(np.uint32) == 0), '%s: an unused slot is not +0.0' % what
    if got.get('spectrum') is not None:
        e = np.abs(np.asarray(got['spectrum'], np.float64) - ref['spectrum'])
        assert np.all(e <= ref['bound']), '%s: spectrum error above its bound' % what
        worst['spectrum'] = float(np.max(e / np.maximum(ref['bound'], 1e-300)))
    return worst


# ---------------------------------------------------------------------------------------------------------------- float32, as stated
def _fma(a, b, c):
    """fmaf: the product of two float32 is exact in float64; the sum is rounded to float64 and then to float32, which is fmaf's single
    rounding unless the float64 sum is inexact AND lands on a float32 tie -- not so for the tie frames, whose sums are exact"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def _dot3(u, g):
    """include/salsa_hip.h: dot = fmaf(u_z, U_z, fmaf(u_y, U_y, u_x U_x))"""
    return _fma(u[..., 2], g[..., 2], _fma(u[..., 1], g[..., 1], u[..., 0] * g[..., 0]))


def kernel_order_float32(v, loc):
    """One FOA label frame in float32, in the operation order include/salsa_hip.h states (salsa_doa_hist): the votes normalised, every
    cell's score summed in vote order, the greedy peaks with the lowest index on a tie (np.argmax takes the first of the largest), the
    refinement summed in vote order.  v float32 (n_cells, 3): channels 4, 5, 6.  -> dict(count, n_votes, cell, score, direction,
    spectrum), float32.  For the frames built to tie: it shows that the tied scores have equal bits, which is not assumed."""
    assert loc.matrix is None
    f, K, G = np.float32, loc.max_sources, loc.n_cells
    v = np.asarray(v, f).reshape(-1, 3)
    Ug, c0, inv = loc.grid, f(loc.c0), f(loc.inv)
    with np.errstate(all='ignore'):
        u = v[:, [2, 0, 1]]
        length = np.sqrt(_fma(u[:, 2], u[:, 2], _fma(u[:, 1], u[:, 1], u[:, 0] * u[:, 0])))
        ok = np.isfinite(v).all(axis=1) & (v != 0).any(axis=1) & (length >= f(loc.norm_lo)) & (length <= f(loc.norm_hi))
        u = (u[ok] / length[ok][:, None]).astype(f)
    sc = np.zeros(G, f)
    for w in u:
        sc = sc + np.maximum(f(0), (_dot3(w, Ug) - c0) * inv)
    assert sc.dtype == f
    out = dict(count=0, n_votes=len(u), cell=np.full(K, -1, np.int32), score=np.zeros(K, f), direction=np.zeros((K, 3), f), spectrum=sc)
    free = np.ones(G, bool)
    for k in range(K):
        if not free.any():
            break
        s = np.where(free, sc, f(-1))
        g = int(np.argmax(s))
        if not s[g] >= f(loc.min_score):
            break
        m = np.zeros(3, f)
        for w in u[_dot3(u, Ug[g]) >= c0]:
            m = m + w
        out['cell'][k], out['score'][k] = g, s[g]
        out['direction'][k] = m / np.sqrt(_fma(m[2], m[2], _fma(m[1], m[1], m[0] * m[0])))
        out['count'] += 1
        free &= ~(_dot3(Ug, Ug[g]) >= f(loc.cos_suppress))
    return out


# ---------------------------------------------------------------------------------------------------------------- built vote sets
def _votes_around(rng, centre_deg, n, spread_deg, length=(0.8, 1.25)):
    """n unit vectors scattered about a direction, each scaled by a length inside the norm range -> float64 (n, 3) (x, y, z)"""
    c = unit(*centre_deg) if len(centre_deg) == 2 else np.asarray(centre_deg, np.float64)
    d = c[None, :] + np.deg2rad(spread_deg) * rng.standard_normal((n, 3))
    d /= np.sqrt((d * d).sum(axis=1, keepdims=True))
    return d * rng.uniform(length[0], length[1], (n, 1))


def _sphere(rng, n):
    d = rng.standard_normal((n, 3))
    return d / np.sqrt((d * d).sum(axis=1, keepdims=True))


def off_grid(loc, az, el):
    """the grid cell at (az, el) moved by (0.3 s, 0.2 s): off every symmetry point of the grid"""
    return (az + 0.3 * loc.grid_step, el + 0.2 * loc.grid_step)


def frame_recipes(loc):
    """{name: (n_cells) -> float64 (n, 3) direction votes (x, y, z), placed by fill_frame}: the frames of the GPU list"""
    s = loc.grid_step
    near = lambda az, el: off_grid(loc, az, el)

    def counted(n):
        return lambda rng, ncells: _votes_around(rng, near(30, 15), min(n, ncells), 3.0)

    def full(rng, ncells):                                                     # every cell votes: two clusters and a thin background
        a, b = min(300, ncells // 4), min(250, ncells // 5)
        v = np.concatenate([_votes_around(rng, near(-60, 30), a, 3.0), _votes_around(rng, near(105, -15), b, 3.0),
                            _sphere(rng, ncells - a - b)])
        return v[rng.permutation(ncells)]

    def two(sep):                                                              # two clusters `sep` degrees apart, on a bearing of 40 degrees:
        c1 = unit(*near(15, 0))                                                # (along a meridian or a parallel the grid has cells at exactly 30)
        az = np.deg2rad(near(15, 0)[0])
        east = np.array([-np.sin(az), np.cos(az), 0.0])
        t = np.cos(np.deg2rad(40.0)) * east + np.sin(np.deg2rad(40.0)) * np.cross(c1, east)
        c2 = np.cos(np.deg2rad(sep)) * c1 + np.sin(np.deg2rad(sep)) * t
        return lambda rng, ncells: np.concatenate([_votes_around(rng, c1, 60, 1.0), _votes_around(rng, c2, 40, 1.0)])

    def threshold(above):                                                      # eight equal votes and a ninth that tips the best score
        def build(rng, ncells):
            d, lo, hi = unit(*near(-90, 45)), 0.0, 40.0
            for _ in range(40):
                mid = 0.5 * (lo + hi)
                ninth = unit(near(-90, 45)[0], near(-90, 45)[1] - mid)
                sc = np.maximum(0.0, (np.vstack([np.tile(d, (8, 1)), ninth]) @ loc.grid.astype(np.float64).T - loc.c0) * loc.inv).sum(axis=0).max()
                lo, hi = (mid, hi) if sc > loc.min_score + (0.05 if above else -0.05) else (lo, mid)
            return np.vstack([np.tile(d, (8, 1)), unit(near(-90, 45)[0], near(-90, 45)[1] - lo)])
        return build

    def dirty(rng, ncells):                                                    # good votes among NaN, Inf and lengths outside the range
        good = _votes_around(rng, near(150, -30), 40, 2.0)
        bad = _votes_around(rng, near(150, -30), 24, 2.0)
        bad[0:4, 0], bad[4:8, 1], bad[8:12, 2] = np.nan, np.inf, -np.inf
        bad[12:18] *= 0.3 / np.sqrt((bad[12:18] ** 2).sum(axis=1, keepdims=True))               # too short
        bad[18:24] *= 3.0 / np.sqrt((bad[18:24] ** 2).sum(axis=1, keepdims=True))               # too long
        v = np.concatenate([good, bad])
        return v[rng.permutation(len(v))]

    def dense(rng, ncells):                                                    # every cell votes, no background: 2500 / 4096 of them in one cap
        a = (2500 * ncells) // 4096
        v = np.concatenate([_votes_around(rng, near(-60, 30), a, 3.0), _votes_around(rng, near(105, -15), ncells - a, 3.0)])
        return v[rng.permutation(ncells)]

    def clusters(n):                                                           # n clusters of 20 + 2 i votes: K = 8 meets eight and nine peaks
        def build(rng, ncells):
            v = np.concatenate([_votes_around(rng, near(*CLUSTER_CENTRES[i]), 20 + 2 * i, 2.0) for i in range(n)])
            return v[rng.permutation(len(v))]
        return build

    def extreme(rng, ncells):                                                  # good votes among lengths that float32 cannot square, or hold
        good = _votes_around(rng, near(150, -30), 40, 2.0)
        bad = _votes_around(rng, near(150, -30), 3 * len(EXTREME_SCALES), 2.0)
        bad *= np.repeat(EXTREME_SCALES, 3)[:, None] / np.sqrt((bad ** 2).sum(axis=1, keepdims=True))
        v = np.concatenate([good, bad])
        return v[rng.permutation(len(v))]

    return {'n0': counted(0), 'n1': counted(1), 'n255': counted(255), 'n256': counted(256), 'n257': counted(257), 'full': full,
            'north': lambda rng, n: _votes_around(rng, (40, 89.2), 50, 1.5), 'south': lambda rng, n: _votes_around(rng, (-70, -89.4), 50, 1.5),
            'seam': lambda rng, n: _votes_around(rng, (179.6, 10 + 0.2 * s), 60, 2.0),
            'apart29': two(29.0), 'apart31': two(31.0), 'above': threshold(True), 'below': threshold(False), 'dirty': dirty,
            'two': lambda rng, n: np.concatenate([_votes_around(rng, near(40, 0), 50, 2.0), _votes_around(rng, near(-100, 20), 30, 2.0)]),
            'n63': counted(63), 'n64': counted(64), 'n65': counted(65), 'full4096': full, 'dense4096': dense,
            'eight': clusters(8), 'nine': clusters(9), 'extreme': extreme}


FRAME_NAMES = ('n0', 'n1', 'n255', 'n256', 'n257', 'full', 'north', 'south', 'seam', 'apart29', 'apart31', 'above', 'below', 'dirty',
               'two', 'n256', 'seam', 'full')                                                   # 18 = two tensors of 3 clips x 3 label frames
CLUSTER_CENTRES = ((45, 35), (-45, 35), (45, -35), (-45, -35), (135, 35), (-135, 35), (135, -35), (-135, -35), (0, 0))
# lengths of the 'extreme' frame's bad votes: float32 flushes the first to zero (a gate) or to a subnormal, the second is subnormal, the
# squares of the next two underflow (to zero, to a subnormal), 1e-10 and 1e10 are plainly out of range, 1e19 squares to 1e38 (the sum
# of three squares may still be finite), the squares of the last three overflow
EXTREME_SCALES = (1e-45, 1e-40, 1e-30, 1e-20, 1e-10, 1e10, 1e19, 1e20, 1e30, 3e38)


def build_features(loc, n_channels=7, n_freq=200, seed=0, names=FRAME_NAMES, clips=3, label_frames=3):
    """len(names) / (clips label_frames) tensors float32 (clips, n_channels, T, n_freq) holding the frames `names` in order, clip-major:
    label_frames label frames of P = loc.frames_per_label feature frames each, and for P > 1 one more, ignored, feature frame (P = 1
    leaves no remainder).  A frame's votes sit at randomly chosen cells of its (P, col1 - col0) window, in order (a recipe that gives
    more votes than the window has cells is cut short); every other cell of the window is a gate, +0.0 or -0.0 at random.  Outside
    the window -- the columns below col0 and from col1 on, the ignored frame -- channels 4-6 hold loud votes toward (0, 0) that must
    not count, channels 0-3 noise, channels beyond 6 NaN.  With the defaults: two tensors (3, n_channels, 25, n_freq) for P = 8."""
    P, ncol = loc.frames_per_label, loc.col1 - loc.col0
    per = clips * label_frames
    assert len(names) % per == 0 and loc.col1 <= n_freq
    T = label_frames * P + (1 if P > 1 else 0)
    D = np.linalg.inv(loc.matrix.astype(np.float64)) if loc.matrix is not None else None
    tensors = []
    for t in range(len(names) // per):
        rng = np.random.default_rng([seed, t, loc.grid_step, ncol])
        x = np.full((clips, n_channels, T, n_freq), np.nan, np.float32)
        x[:, :4] = rng.standard_normal((clips, 4, T, n_freq)).astype(np.float32)
        x[:, 4:7] = _encode(np.tile(unit(0.0, 0.0), (clips * T * n_freq, 1)), D).reshape(clips, T, n_freq, 3).transpose(0, 3, 1, 2)
        for i in range(per):
            b, f = divmod(i, label_frames)
            name = names[per * t + i]
            votes = frame_recipes(loc)[name](np.random.default_rng([seed, t, i, loc.grid_step, ncol]), P * ncol)[:P * ncol]
            win = np.zeros((P * ncol, 3), np.float32)
            win[rng.random((P * ncol, 3)) < 0.5] = -0.0
            at = np.sort(rng.choice(P * ncol, len(votes), replace=False))
            win[at] = _encode(votes, D)
            x[b, 4:7, f * P:(f + 1) * P, loc.col0:loc.col1] = win.reshape(P, ncol, 3).transpose(2, 0, 1)
        tensors.append(x)
    return tensors


def _encode(d, D):
    """direction votes (x, y, z) -> channels (4, 5, 6), float32: FOA (y, z, x); MIC D d, the path differences in metres"""
    d = np.asarray(d, np.float64)
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        return (d @ D.T if D is not None else d[:, [1, 2, 0]]).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- plane waves
def plane_wave_audio(bank, bands=None, seconds=2.0, fs=24000, seed=0):
    """One source per response of `bank` (scenes.make_rir_bank), all sounding for the whole clip: AR(1)-filtered noise (pole 0.9),
    band-limited to bands[i] = (lo, hi) Hz where given, convolved with the response, in white noise of 0.001 -> float32 (4, N)"""
    rng = np.random.default_rng(seed)
    N = int(seconds * fs)
    audio = 0.001 * rng.standard_normal((4, N))
    for i in range(bank.n_rirs):
        w = rng.standard_normal(N)
        s = np.zeros(N)
        acc = 0.0
        for n in range(N):
            acc = 0.9 * acc + w[n]
            s[n] = acc
        s /= s.std()
        if bands is not None:
            S = np.fft.rfft(s)
            fr = np.fft.rfftfreq(N, 1.0 / fs)
            S[(fr < bands[i][0]) | (fr > bands[i][1])] = 0.0
            s = np.fft.irfft(S, N)
            s /= s.std()
        for c in range(4):
            audio[c] += 0.1 * np.convolve(s, bank.rirs[i, c].astype(np.float64))[:N]
    return audio.astype(np.float32)
