"""The N-microphone (5 - 16) eigen-solver of the contrib surface against LAPACK, on the CPU.

Matrix level: salsa_math.h hermn_gate_eigvec -- the statements cov_eig_n_kernel runs per TF bin, compiled with g++ through
tests/hostemu -- against np.linalg.eigh(UPLO='U') on the built families of tests/flex_families.py: gate decision, eigenvalues,
angle(conj(u_0) u_c), sweeps used and the residual at exit, through the unrolled instantiations (6, 8) and the run-time-sized one.
Oracle level: oracle.flexible (its own cyclic Jacobi, another stop rule) against tests/flex_reference.py (LAPACK) on the audio
families, by the rules the GPU module uses.  The constants of both levels are measured from the reference alone, and re-measured
here.  Run with -s to see the figures."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import flex_families as ff
import flex_reference as fr

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'hostemu', 'hostemu.cpp')
SO = os.path.join(HERE, 'hostemu', 'libhostemu.so')
HDR = os.path.join(os.path.dirname(HERE), 'salsa_amd', 'csrc', 'salsa_math.h')

GATE_MARGIN = 1e-12     # the gate decision equals LAPACK's wherever |m| exceeds this (what the 4 x 4 float64 gate is held to)
# eigh against eigh of the same matrix under a random Hermitian perturbation of norm 2^-52 ||A||, largest error / kappa over all
# families, sizes and seeds (eigenvalues: kappa = ||A||; phases: kappa_c); measured 2.22e-15 (test_delta_mat_... prints it),
# rounded up.  The solver is another backward-stable algorithm, not a re-run: it gets 8 x.
DELTA_MAT = 2.3e-15
MAT_MARGIN = 8.0
STOP_RULE = 1e-34       # off <= STOP_RULE * tr^2 (salsa_math.h hermn_gate_eigvec)

CTOR = dict(fs=ff.FS, stft_winsize=512, hop_length=300, fmin_doa=50, fmax_doa=2000, fmax_spec=9000)
PERTURB_SEEDS = (1, 2, 3)


@pytest.fixture(scope='module')
def emu():
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-o', SO, SRC])
    L = C.CDLL(SO)
    L.hostemu_hermn.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_double, C.c_int] + [C.c_void_p] * 6
    return L


def solve(emu, A, thresh, unrolled):
    A = np.ascontiguousarray(A, np.complex128)
    m, n, _ = A.shape
    o = dict(lam=np.zeros((m, n)), u=np.zeros((m, n), np.complex128), good=np.zeros(m, np.int32), sweeps=np.zeros(m, np.int32),
             off=np.zeros(m), tr=np.zeros(m))
    rc = emu.hostemu_hermn(A.ctypes.data, m, n, thresh, int(unrolled), *[o[k].ctypes.data for k in ('lam', 'u', 'good', 'sweeps', 'off', 'tr')])
    assert rc == 0, (n, unrolled)
    o['good'] = o['good'].astype(bool)
    return o


def lapack(A):
    w, v = np.linalg.eigh(A, UPLO='U')
    u = v[..., :, -1]
    nrm = np.abs(w).max(axis=-1)
    safe = np.where(nrm > 0, nrm, 1.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        g = (w[:, -1] - w[:, -2]) / safe
        kappa = 1.0 / (g[:, None] * np.abs(u[:, :1]) * np.abs(u[:, 1:]))
        kappa = np.where(np.isfinite(kappa), kappa, np.inf)
    return w, u, safe, kappa


def phase(u):
    return np.angle(u[:, :1].conj() * u[:, 1:])


def wrapped(d):
    return d - 2 * np.pi * np.round(d / (2 * np.pi))


def phase_err_over_kappa(u, v, kappa):
    """largest |angle difference| / kappa_c over the elements whose kappa is finite"""
    with np.errstate(invalid='ignore'):
        e = np.abs(wrapped(phase(u) - phase(v))) / kappa
    return float(np.where(np.isfinite(kappa), e, 0.0).max(initial=0.0))


def all_matrices():
    for name in sorted(ff.MATRIX_FAMILIES):
        for N in ff.MATRIX_N:
            for thr in ff.THRESHOLDS:
                yield name, N, thr, ff.matrices(name, N, thr)


def measure_delta_mat():
    worst = {}
    for name, N, thr, A in all_matrices():
        w, u, nrm, kappa = lapack(A)
        for seed in PERTURB_SEEDS:
            rng = np.random.RandomState(seed)
            E = rng.randn(*A.shape) + 1j * rng.randn(*A.shape)
            E = (E + E.conj().swapaxes(-1, -2)) / 2
            E /= np.linalg.norm(E, 2, axis=(-2, -1))[:, None, None]
            w2, u2, _, _ = lapack(A + 2.0 ** -52 * np.where(np.abs(w).max(axis=-1) > 0, nrm, 0.0)[:, None, None] * E)
            e = max(float((np.abs(w2 - w).max(axis=-1) / nrm).max()), phase_err_over_kappa(u, u2, kappa))
            worst[name] = max(worst.get(name, 0.0), e)
    return worst


def test_delta_mat_is_not_below_what_lapack_does_to_itself():
    worst = measure_delta_mat()
    for name in sorted(worst):
        print('delta_mat %-12s %.3e' % (name, worst[name]))
    print('delta_mat measured %.3e, constant %.3e' % (max(worst.values()), DELTA_MAT))
    assert DELTA_MAT >= max(worst.values())


def instantiations(n):
    return (0, 1) if n in (6, 8) else (0,)


@pytest.mark.parametrize('name', sorted(ff.MATRIX_FAMILIES))
def test_solver_against_lapack_on_built_matrices(emu, name):
    """Gate = LAPACK's wherever |m| > 1e-12 (and on the exact ties of `exact_tie`, which '>' fails); eigenvalues within
    8 DELTA_MAT ||A||, angle(conj(u_0) u_c) within 8 DELTA_MAT kappa_c where both gates pass; every solve leaves by the stop rule
    (sweeps below the cap, or the residual meets the rule anyway)."""
    cap = emu.hostemu_hermn_sweep_cap()
    n_mat = n_sure = n_gated = 0
    worst_ev = worst_ph = 0.0
    most_sweeps = 0
    for N in ff.MATRIX_N:
        for thr in ff.THRESHOLDS:
            A = ff.matrices(name, N, thr)
            w, u, nrm, kappa = lapack(A)
            pos = w[:, -1] > 0
            m = np.where(pos, (w[:, -1] - thr * w[:, -2]) / np.where(pos, w[:, -1], 1.0), -1.0)
            ref_good = w[:, -1] > w[:, -2] * thr
            sure = np.abs(m) > GATE_MARGIN
            if name == 'exact_tie':                                   # exact arithmetic on both sides: the tie itself is held
                assert (w[:, -1] == w[:, -2] * thr).all() and not ref_good.any()
                sure[:] = True
            for unrolled in instantiations(A.shape[-1]):
                s = solve(emu, A, thr, unrolled)
                what = (name, N, thr, unrolled)
                assert np.array_equal(s['good'][sure], ref_good[sure]), (what, m[sure][s['good'][sure] != ref_good[sure]])
                ev = np.abs(s['lam'] - w).max(axis=-1) / nrm
                assert ev.max() <= MAT_MARGIN * DELTA_MAT, (what, float(ev.max()))
                both = s['good'] & ref_good
                ph = phase_err_over_kappa(u[both], s['u'][both], kappa[both]) if both.any() else 0.0
                assert ph <= MAT_MARGIN * DELTA_MAT, (what, ph)
                assert not np.abs(s['u'][~s['good']]).any()
                by_cap = (s['sweeps'] >= cap) & ~(s['off'] <= STOP_RULE * s['tr'] * s['tr'])
                assert not by_cap.any(), (what, 'left by the sweep cap with residual', s['off'][by_cap] / s['tr'][by_cap] ** 2)
                assert (s['sweeps'][s['tr'] <= 0] == 0).all() and not s['good'][s['tr'] <= 0].any()
                n_mat += len(A)
                n_sure += int(sure.sum())
                n_gated += int(both.sum())
                worst_ev, worst_ph, most_sweeps = max(worst_ev, float(ev.max())), max(worst_ph, ph), max(most_sweeps, int(s['sweeps'].max()))
    print('%-12s %5d solves, %5d with |m| > 1e-12, %5d gated | eigenvalues %.2e ||A||, phases %.2e kappa (bound %.2e) | sweeps <= %d of %d'
          % (name, n_mat, n_sure, n_gated, worst_ev, worst_ph, MAT_MARGIN * DELTA_MAT, most_sweeps, cap))
    assert n_mat > 0 and (n_sure > 0.5 * n_mat or name == 'knife_edge')


def test_unrolled_and_run_time_sized_instantiations_agree_bit_for_bit(emu):
    """hermn<6> / hermn<8> and hermn<0> at the same size run the same statements: same bits out (the kernel's instantiations differ
    in addressing only)."""
    for name in sorted(ff.MATRIX_FAMILIES):
        for N in (5, 6, 7, 8):
            A = ff.matrices(name, N, 4.0)
            a, b = solve(emu, A, 4.0, 0), solve(emu, A, 4.0, 1)
            for k in a:
                assert np.array_equal(a[k], b[k]), (name, N, k)


# ------------------------------------------------------------------------------------------------------------ audio level
_cache = {}


def spectra(oracle, name, n_ch, seed=0):
    key = (name, n_ch, seed)
    if key not in _cache:
        y = ff.audio(name, n_ch, seed)
        X = np.stack([oracle.stft(y[c], CTOR['stft_winsize'], CTOR['hop_length']) for c in range(n_ch)])
        _cache[key] = (y, X, fr.decompose(X, 3))
    return _cache[key]


def call_of(thr, trk):
    return dict(clip_freqs=trk, clip_spatial_alias=bool(trk and thr == 4.0), ew_thresh=thr, covmat_avg_neighbours=3, is_tracking=trk, floor_mask_ratio=1.5)


def family_pairs():
    return sorted({(name, n_ch) for name, n_ch, _, _ in ff.audio_cases()})


def measure_ulp_constants(oracle):
    """The reference against itself on spectra moved by one float32 ulp per component: the largest |m| at which its gate decision
    flips (any threshold of the suite, every bin, tracker aside) and the largest phase change / kappa_c on elements gated both
    times.  Flips are rare (none in the ~3e6 decisions here), so the largest CHANGE of m is taken too: a flip needs m to change
    sign, i.e. |m| <= |change of m|.  -> (largest flipped |m|, largest |change of m|, flips, largest err / kappa, tracker-mask
    differences)"""
    m_flip, n_flip, worst, trk_diff, dm = 0.0, 0, 0.0, 0, 0.0
    for name, n_ch in family_pairs():
        _, X, dec = spectra(oracle, name, n_ch)
        for seed in PERTURB_SEEDS:
            Xp = fr.ulp_perturbed(X, seed)
            decp = fr.decompose(Xp, 3)
            for thr in ff.THRESHOLDS:
                a = fr.features(X, dec, CTOR, call_of(thr, False))
                b = fr.features(Xp, decp, CTOR, call_of(thr, False))
                flip = a['good'] != b['good']
                live = (dec['l1'] > 0) & (decp['l1'] > 0)
                dm = max(dm, float(np.abs(a['m'] - b['m'])[live[a['lo']:a['lo'] + len(a['m'])]].max()))
                if flip.any():
                    n_flip += int(flip.sum())
                    m_flip = max(m_flip, float(np.abs(a['m'][flip]).max()))
                if thr == min(ff.THRESHOLDS):                       # the widest set of gated bins
                    both = np.broadcast_to((a['good'] & b['good'])[None], a['kappa'].shape) & np.isfinite(a['kappa']) & (a['kappa'] > 0)
                    with np.errstate(invalid='ignore'):
                        e = np.abs(wrapped(a['phase'] - b['phase'])) / a['kappa']
                    worst = max(worst, float(np.where(both, e, 0.0).max(initial=0.0)))
            ta = fr.features(X, dec, CTOR, call_of(5.0, True))['evaluated']
            tb = fr.features(Xp, decp, CTOR, call_of(5.0, True))['evaluated']
            trk_diff += int((ta != tb).sum())
    return m_flip, dm, n_flip, worst, trk_diff


def test_doubt_band_and_delta_stft_are_not_below_the_reference_s_own_sensitivity(oracle):
    m_flip, dm, n_flip, worst, trk_diff = measure_ulp_constants(oracle)
    print('1-ulp perturbation of the spectra: %d gate flips, largest |m| at a flip %.3e, largest change of m %.3e -> m_band %.3e '
          '(constant %.3e); largest phase change / kappa %.3e -> delta_stft %.3e (constant %.3e); tracker mask differences %d'
          % (n_flip, m_flip, dm, 2 * max(m_flip, dm), fr.M_BAND, worst, 4 * worst, fr.DELTA_STFT, trk_diff))
    assert fr.M_BAND >= 2 * max(m_flip, dm)
    assert fr.DELTA_STFT >= 4 * worst
    # the rules have no doubt band for the tracker's own comparisons: the families are built clear of its knife edges
    assert trk_diff == 0


@pytest.mark.parametrize('name', sorted(ff.AUDIO_FAMILIES))
def test_oracle_against_lapack_reference_on_audio_family(oracle, name):
    """oracle.flexible (cyclic Jacobi, 80 sweeps) against the LAPACK reference on the oracle's own STFT of the family's clips, by
    the GPU module's rules; and the conditions the rules put on the families, met by the reference alone: at most 1e-3 of a case's
    compared bins inside the doubt band, at most 1 % of the family's gated elements left out of the value comparison."""
    gated = excluded = 0
    worst_tight = 0.0
    for fam, n_ch, thr, trk in ff.audio_cases():
        if fam != name:
            continue
        y, X, dec = spectra(oracle, name, n_ch)
        call = call_of(thr, trk)
        ref = fr.features(X, dec, CTOR, call)
        out = oracle.flexible(y, kind='salsa', **CTOR, **call)
        real_tf = fr.real_spectrum_bins(ref['gate'].shape[0], ref['gate'].shape[1], ref['lo'], CTOR['stft_winsize'], y.shape[1],
                                        CTOR['hop_length'])
        np.testing.assert_allclose(out[:n_ch], ref['spec_db'], rtol=1e-5, atol=2e-5)
        what = '%s n_ch %d thresh %g tracking %s' % (name, n_ch, thr, trk)
        st = fr.compare(out[n_ch:], ref, real_tf, trk, what=what)
        # the GPU's rules allow for spectra that differ in the last bit; the oracle sees the reference's own spectra, so its Jacobi
        # is also held to LAPACK as the host-emulated solver is: |dphase| <= 8 DELTA_MAT kappa_c on everything gated
        tight = fr.compare(out[n_ch:], ref, real_tf, trk, delta_stft=MAT_MARGIN * DELTA_MAT, what=what + ' (matrix-level bound)')
        worst_tight = max(worst_tight, tight['worst'])
        share = st['in_band'] / max(1, st['compared'])
        print('%-17s n_ch %2d thresh %4g tracking %-5s: %6d bins compared, %d in the doubt band (%.1e), %7d gated elements, '
              '%d left out, worst |dphase| %.2e rad = %.3f of its bound'
              % (name, n_ch, thr, trk, st['compared'], st['in_band'], share, st['gated'], st['excluded'], st['max_err'], st['worst']))
        assert share <= fr.DOUBT_SHARE_MAX
        gated += st['gated']
        excluded += st['excluded']
    print('%-17s left out of the value comparison: %d of %d gated elements (%.2e); worst |dphase| = %.3f of 8 DELTA_MAT kappa_c'
          % (name, excluded, gated, excluded / max(1, gated), worst_tight))
    if name == 'silent_ch0':
        assert gated == 0          # u_0 = 0: every phase is angle(0) = 0; gates and the exact-zero pattern are what is held
    else:
        assert gated > 1000 and excluded <= fr.EXCLUDED_SHARE_MAX * gated
