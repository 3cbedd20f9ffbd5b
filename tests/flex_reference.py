"""Float64 restatement of the contrib on-the-fly SALSA features (contrib/salsa_flexible.py SalsaFeatures) with LAPACK as the
eigen-solver.  TEST INFRASTRUCTURE: plain numpy, written from the behaviour oracle/salsa_oracle.c documents (contrib :52-77,
:118-146, :316-367).  Unlike the oracle and the HIP kernel (both cyclic Jacobi) the N x N Hermitian problem goes to
np.linalg.eigh(UPLO='U') -- the reference's own call -- so this module is the independent solver the N-microphone path is held to.

    d = decompose(X, covmat_avg_neighbours)          # X [C][nb][T] complex64 spectra (all n_fft/2+1 bins)
    r = features(X, d, ctor, call)                   # spat [C-1][F][T] + per-bin diagnostics

Per TF bin, besides the features: the gate margin m = (l1 - thresh * l2) / l1, the gap g = (l1 - l2) / l1, |u_c| of the top
eigenvector and the conditioning kappa_c = 1 / (g |u_0| |u_c|) of angle(conj(u_0) u_c): a perturbation of relative size d of the
covariance turns the top eigenvector by ~ d / g, which moves the phase of a component of modulus |u_c| by ~ d / (g |u_c|)."""
import numpy as np

SOUND_SPEED = 343.0


def bin_limits(fs, n_fft, fmin_doa, fmax_doa, fmax_spec):
    lower = max(1, int(np.floor(fmin_doa * n_fft / float(fs))))
    upper = int(np.floor(fmax_doa * n_fft / float(fs)))
    cutoff = int(np.floor(fmax_spec * n_fft / float(fs)))
    assert upper <= cutoff
    return lower, upper, cutoff


def norm_freq(fs, n_fft):
    """float32 arange, entry 0 set to 1, scaled IN float32 by delta (:185-187) -> float64 [nb]"""
    nf = np.arange(n_fft // 2 + 1, dtype=np.float32)
    nf[0] = 1
    nf *= 2 * np.pi * fs / (n_fft * SOUND_SPEED)
    return nf.astype(np.float64)


def covariances(X, neigh):
    """X [C][nb][T] complex -> [nb][T][C][C] complex128: SUM over the 2 * neigh + 1 frames around t (wrap on the time axis) of
    x_i conj(x_j)."""
    Xd = np.ascontiguousarray(np.transpose(X, (1, 2, 0))).astype(np.complex128)           # [nb][T][C]
    R = np.zeros(Xd.shape + (Xd.shape[-1],), np.complex128)
    for k in range(-neigh, neigh + 1):
        Xk = np.roll(Xd, -k, axis=1)                                                   # frame t + k at position t
        R += Xk[..., :, None] * Xk[..., None, :].conj()
    return R


def decompose(X, neigh=3):
    """LAPACK on every bin's covariance: the two largest eigenvalues and the top eigenvector (what the features depend on)."""
    R = covariances(X, neigh)
    w, v = np.linalg.eigh(R, UPLO='U')
    return dict(l1=w[..., -1], l2=w[..., -2], u=np.ascontiguousarray(np.moveaxis(v[..., :, -1], -1, 0)), lam=w)   # u [C][nb][T]


def tracker_mask(mag, floor_mask_ratio=1.5, steps=3, up_initial=1.02, up_many=1.002, down=0.98, epsilon=1e-6):
    """The contrib noise-floor tracker (:80-146) on |X_0| [nb][T]: initial floor = half the mean of the first five frames, clamped
    to epsilon; per frame the floor rises by up_initial (first `steps` consecutive frames above it) or up_many (later ones), sinks
    by `down` otherwise, is clamped again, and the mask is mag > ratio * UPDATED floor."""
    nb, T = mag.shape
    floor = 0.5 * np.mean(mag[:, 0:5], axis=1)
    floor = np.maximum(floor, epsilon)
    count = np.zeros(nb, np.int64)
    mask = np.zeros((nb, T), bool)
    for t in range(T):
        above = mag[:, t] > floor
        count += above
        few, many = above & (count <= steps), above & (count > steps)
        floor = np.where(few, floor * up_initial, floor)
        floor = np.where(many, floor * up_many, floor)
        floor = np.where(~above, floor * down, floor)
        floor = np.maximum(floor, epsilon)
        count[~above] = 0
        mask[:, t] = mag[:, t] > floor_mask_ratio * floor
    return mask


def features(X, dec, ctor, call):
    """ctor: fs, stft_winsize, fmin_doa, fmax_doa, fmax_spec; call: clip_freqs, clip_spatial_alias, ew_thresh,
    covmat_avg_neighbours (must be what `dec` was made with), is_tracking, floor_mask_ratio.
    -> dict: spat [C-1][F][T] float64, spec_db [C][F][T] float64, evaluated / good / gate [F][T] bool (gate = evaluated & good =
    what reaches the output), m, g [F][T], uabs [C][F][T], kappa [C-1][F][T], nf [F], lo, alias_from."""
    fs, n_fft = ctor['fs'], ctor['stft_winsize']
    nb = n_fft // 2 + 1
    lower, upper, cutoff = bin_limits(fs, n_fft, ctor['fmin_doa'], ctor['fmax_doa'], ctor['fmax_spec'])
    lo, hi = (lower, min(cutoff, nb)) if call.get('clip_freqs', True) else (0, nb)
    thresh = float(call.get('ew_thresh', 5.0))
    sl = slice(lo, hi)
    l1, l2, u = dec['l1'][sl], dec['l2'][sl], dec['u'][:, sl].copy()
    u[~np.asarray(X).reshape(len(X), -1).any(axis=1)] = 0   # a silent channel: zero row and column, component 0 whatever LAPACK leaves
    nf = norm_freq(fs, n_fft)[sl]
    good = l1 > l2 * thresh
    mag = np.abs(X[0, sl].astype(np.complex128))
    if call.get('is_tracking', True):
        evaluated = tracker_mask(mag, call.get('floor_mask_ratio', 1.5))
    else:   # one all-pass mask narrowed in place: a bin is evaluated while every earlier frame of it passed
        evaluated = np.concatenate([np.ones_like(good[:, :1]), np.logical_and.accumulate(good, axis=1)[:, :-1]], axis=1)
    gate = evaluated & good
    with np.errstate(divide='ignore', invalid='ignore'):
        pos = l1 > 0
        m = np.where(pos, (l1 - thresh * l2) / np.where(pos, l1, 1.0), -1.0)
        g = np.where(pos, (l1 - l2) / np.where(pos, l1, 1.0), 0.0)
        uabs = np.abs(u)
        kappa = 1.0 / (g[None] * uabs[0][None] * uabs[1:])
    phase = np.angle(u[0][None].conj() * u[1:])
    spat = np.where(gate[None], phase / nf[None, :, None], 0.0)
    alias_from = upper if call.get('clip_spatial_alias', False) else None     # index into the (possibly cropped) axis (:263)
    if alias_from is not None:
        spat[:, alias_from:] = 0
    p = np.abs(X[:, sl].astype(np.complex128)) ** 2
    spec_db = 10.0 * np.log10(np.maximum(1e-10, p))
    return dict(spat=spat, spec_db=spec_db, evaluated=evaluated, good=good, gate=gate, m=m, g=g, uabs=uabs, kappa=kappa, nf=nf,
                lo=lo, alias_from=alias_from, phase=phase)


def ulp_perturbed(X, seed):
    """X complex64 with every real and imaginary component moved by one float32 ulp up or down (seeded coin per component).
    Exact zeros stay: the spectrum of digital silence is 0 in any float32 STFT, not 0 to within an ulp."""
    rng = np.random.RandomState(seed)
    f = np.ascontiguousarray(X, np.complex64).view(np.float32)
    up = rng.randint(0, 2, f.shape).astype(bool)
    out = np.where(up, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))).astype(np.float32)
    return np.where(f == 0, f, out).view(np.complex64)


# ------------------------------------------------------------------------------------------------------ comparison rules
# An implementation fed float32 spectra that may differ from these in the last bit (the HIP STFT against the oracle's) is held to
# this reference by rules whose two constants are measured FROM THE REFERENCE ALONE (tests/test_flex_solver_cpu.py re-measures
# them): the reference against itself on spectra with every component moved by one float32 ulp.
#   M_BAND      twice the largest |m| at which the reference's own gate decision flipped under that perturbation -- or could
#               have: a flip needs m to change sign, so the largest change of m it saw bounds every flip's |m|;
#   DELTA_STFT  four times the largest phase change / kappa_c it saw on elements gated both times.
M_BAND = 2.2e-6
DELTA_STFT = 2.5e-7
DOUBT_SHARE_MAX = 1e-3      # of the compared bins of a case may lie inside the doubt band
BOUND_MAX = 1e-3            # rad: elements whose bound kappa_c * DELTA_STFT exceeds this are left out of the value comparison ...
EXCLUDED_SHARE_MAX = 1e-2   # ... and may be at most this share of a family's gated elements
SILENT_SHOWN_MIN = 0.99     # of the passing bins that only a silent channel's round-off can show (pair-packed STFT) are non-zero


def real_spectrum_bins(F, T, lo, n_fft, n_samples, hop):
    """The rule of tests/flex_compare.py: frame 0, a last frame centred on the last sample, bins 0 and n_fft / 2 have spectra that
    are real up to round-off; a 0-or-+-pi phase there has its sign decided by that round-off."""
    k = np.arange(lo, lo + F)
    real_tf = np.zeros((F, T), bool)
    real_tf[:, 0] = True
    if (n_samples - 1) % hop == 0 or n_samples % hop == 0:
        real_tf[:, -1] = True
    real_tf[(k == 0) | (k == n_fft // 2), :] = True
    return real_tf


def doubt(ref, is_tracking, m_band=None):
    """[F][T] bool: bins whose gate the rules do not pin: an evaluated bin with |m| <= m_band -- and, with is_tracking=False,
    every later frame of that bin (the all-pass mask is narrowed in place: one decision carries to the end of the clip)."""
    m_band = M_BAND if m_band is None else m_band
    d = ref['evaluated'] & (np.abs(ref['m']) <= m_band)
    if not is_tracking:
        d = np.logical_or.accumulate(d, axis=1)
    return d


def compare(spat, ref, real_tf, is_tracking, m_band=None, delta_stft=None, what='', silent_exact=True):
    """spat [C-1][F][T] (the implementation's spatial planes) against features(...) `ref`.  Asserts the gate pattern, the
    exact-zero pattern and the values; returns the counts the shares are made of."""
    m_band = M_BAND if m_band is None else m_band
    delta_stft = DELTA_STFT if delta_stft is None else delta_stft
    spat = np.asarray(spat, np.float64)
    assert spat.shape == ref['spat'].shape, (spat.shape, ref['spat'].shape)
    assert np.isfinite(spat).all(), what
    F, T = ref['gate'].shape
    visible = ref['gate'].copy()                      # what the output can show of the gate
    if ref['alias_from'] is not None:
        visible[ref['alias_from']:] = False
    zero_elem = np.broadcast_to((ref['uabs'][0] == 0)[None] | (ref['uabs'][1:] == 0), spat.shape)
    shown = visible & (~zero_elem).any(axis=0)        # bins at which a passing gate MUST show as a non-zero value
    dbt = doubt(ref, is_tracking, m_band)
    generic = ~real_tf & ~dbt
    got = (spat != 0).any(axis=0)
    gate_bad = ((got & ~visible) | (shown & ~got)) & generic
    assert not gate_bad.any(), '%s: gate pattern differs outside the doubt band at %d bins, |m| there >= %.3e' % (
        what, int(gate_bad.sum()), float(np.abs(ref['m'][gate_bad]).min()))
    # a silent channel (c or 0): conj(u_0) u_c is a signed zero, whose angle is 0 or +-pi by the signs alone.  That much holds
    # where the channel's spectrum IS zero (silent_exact=True: the oracle); the passing side of a gate that only silent elements
    # could show ("silent channel 0") is then not observable in the output, and is held nowhere.  An STFT that transforms real
    # channels in pairs (the HIP one, silent_exact=False) leaves a silent channel the round-off of its partner instead: its phase
    # is as meaningless as that sign and no value is held, but it is a NON-ZERO phase, so there the passing side is held by a
    # share: at least SILENT_SHOWN_MIN of the passing bins that only silent elements can show do show.
    hidden = visible & ~shown & generic
    silent_shown = float(got[hidden].mean()) if hidden.any() else 1.0
    if silent_exact:
        z = np.abs(spat * ref['nf'][None, :, None])[zero_elem]
        assert np.all((z == 0) | (np.abs(z - np.pi) <= 1e-6)), '%s: a silent channel has a phase that is neither 0 nor +-pi' % what
    else:
        assert silent_shown >= SILENT_SHOWN_MIN, '%s: only %.4f of the passing bins of silent elements show a value' % (what, silent_shown)
    if ref['alias_from'] is not None:
        assert not (spat[:, ref['alias_from']:] != 0).any(), what
    if not is_tracking:                               # once a bin fails, all its later frames are exactly 0 in every plane
        rows = ~real_tf.all(axis=1)                   # (bins 0 and n_fft / 2: phases of exactly 0 are values there, not failures)
        # a passing bin of silent elements alone may have nothing to show (0 is a legitimate angle of a zero; on the GPU too, where
        # the round-off left in a silent channel is now and then exactly 0 over a whole window): it is counted from the reference
        seen = got | (visible & ~shown)
        assert np.array_equal(seen[rows], np.logical_and.accumulate(seen, axis=1)[rows]), '%s: a bin came back after it failed' % what
    # Elements of a silent channel (kappa_c infinite) are taken out HERE, before the excluded share is counted: the issue's
    # accounting would count them as left out (1 / (C - 1) of "silent middle channel", every element of "silent channel 0"); they
    # are held by the rules above instead (0 or +-pi; finite and, on the GPU, the share) and the 1 % is asked of the other elements.
    both = np.broadcast_to((got & shown & ~dbt)[None], spat.shape) & ~zero_elem
    bound = ref['kappa'] * delta_stft
    with np.errstate(invalid='ignore'):
        held = both & (bound <= BOUND_MAX)
    d = (spat - ref['spat']) * ref['nf'][None, :, None]                      # phase difference, rad
    dw = d - 2 * np.pi * np.round(d / (2 * np.pi))
    err = np.abs(np.where(real_tf[None], dw, d))
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where(held, err / bound, 0.0)
    assert ratio.max(initial=0.0) <= 1.0, '%s: |dphase| = %.3e x its bound kappa_c * delta_stft (kappa %.3e)' % (
        what, float(ratio.max()), float(ref['kappa'].ravel()[ratio.argmax()]))
    compared = int((~real_tf).sum())
    return dict(compared=compared, silent_shown=silent_shown, hidden=int(hidden.sum()), in_band=int((dbt & ~real_tf).sum()), gated=int(both.sum()), excluded=int((both & ~held).sum()),
                worst=float(ratio.max(initial=0.0)), max_err=float(np.where(held, err, 0.0).max(initial=0.0)))
