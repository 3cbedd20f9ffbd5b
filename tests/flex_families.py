"""Built inputs for the N-microphone (5 - 16) eigen-solver of the contrib surface (cov_eig_n_kernel / hermn_gate_eigvec).
TEST INFRASTRUCTURE.  Two kinds, both seeded and deterministic:

* MATRIX families: N x N Hermitian matrices handed straight to the host-emulated solver (tests/test_flex_solver_cpu.py).  Odd N
  is embedded with a zero last row and column, as salsa_amd/flexible.py pads an odd microphone count with a silent channel.
* AUDIO families: (n_ch, n) float32 clips that go through the STFT (oracle's on the CPU, the HIP one on the GPU).  All sources are
  white (every bin carries energy, so a float32 STFT resolves every bin to a relative ulp), placed by integer circular delays.

Each family carries a one-line description (MATRIX_FAMILIES / AUDIO_FAMILIES)."""
import numpy as np

THRESHOLDS = (1.05, 4.0, 5.0)
MATRIX_N = tuple(range(5, 17))


def embed(A):
    """[m][N][N] -> [m][N + (N & 1)][...]: zero last row and column for odd N"""
    N = A.shape[-1]
    if N % 2 == 0:
        return A
    out = np.zeros(A.shape[:-2] + (N + 1, N + 1), A.dtype)
    out[..., :N, :N] = A
    return out


def _herm(R):
    return (R + np.conj(np.swapaxes(R, -1, -2))) / 2


def _unitary(rng, N, first=None):
    M = rng.randn(N, N) + 1j * rng.randn(N, N)
    if first is not None:
        M[:, 0] = first
    Q, r = np.linalg.qr(M)
    if first is not None:
        Q[:, 0] *= r[0, 0] / abs(r[0, 0])        # QR leaves column 0 = first / (|first| e^{i arg r00}): put the phases back
    return Q


def _from_spectrum(rng, lam, first=None):
    Q = _unitary(rng, len(lam), first)
    return _herm((Q * np.asarray(lam, float)) @ Q.conj().T)


def _tail(rng, N, top, k):
    """N - k eigenvalues spread below `top`"""
    return list(np.sort(rng.uniform(0.0, 0.8 * top, N - k))[::-1])


def _rank1(rng, N, thresh):
    out = []
    for _ in range(6):
        v = rng.randn(N) + 1j * rng.randn(N)
        out.append(np.outer(v, v.conj()))
    return out


def _rank1_eps(rng, N, thresh):
    out = []
    for eps in 10.0 ** np.arange(-16, -1):
        v = rng.randn(N) + 1j * rng.randn(N)
        v /= np.linalg.norm(v)
        out.append(np.outer(v, v.conj()) + eps * np.eye(N))
    return out


def _knife_edge(rng, N, thresh):
    out = []
    for k in range(10, 51):
        for sign in (-1.0, 1.0):
            l2 = 1.0 / (thresh * (1.0 + sign * 2.0 ** -k))
            out.append(_from_spectrum(rng, [1.0, l2] + _tail(rng, N, l2, 2)))
    return out


def _multiple_top(rng, N, thresh):
    return [_from_spectrum(rng, [1.0] * k + _tail(rng, N, 1.0, k)) for k in (2, 3, N // 2, N) for _ in range(2)]


def _nm1_equal(rng, N, thresh):
    out = []
    for a in (0.5, 0.21, 0.19, 1e-3, 1e-9):
        out.append(_from_spectrum(rng, [1.0] + [a] * (N - 1)))           # one on top of N - 1 equal ones
        out.append(_from_spectrum(rng, [1.0] * (N - 1) + [a]))           # N - 1 equal ones on top
    return out


def _geometric(decades):
    def f(rng, N, thresh):
        return [_from_spectrum(rng, 10.0 ** (-decades * np.arange(N) / (N - 1.0))) for _ in range(4)]
    return f


def _graded(rng, N, thresh):
    out = []
    for k in range(4):
        X = rng.randn(N, 7 + 3 * k) + 1j * rng.randn(N, 7 + 3 * k)
        d = np.logspace(0, -4, N)
        if k & 1:
            d = d[rng.permutation(N)]
        out.append(_herm((X @ X.conj().T) * np.outer(d, d)))
    return out


def _duplicated(rng, N, thresh):
    out = []
    for k in range(4):
        X = rng.randn(N, 7) + 1j * rng.randn(N, 7)
        X[:, 0] *= 4.0
        i, j = rng.choice(N, 2, replace=False)
        X[j] = X[i]
        if k >= 2:
            X[(j + 1) % N if (j + 1) % N != i else (j + 2) % N] = X[i]
        out.append(X @ X.conj().T)
    return out


def _zero(rng, N, thresh):
    return [np.zeros((N, N), complex)]


def _wilkinson(rng, N, thresh):
    """W_M^+ (diagonal |i - (M - 1) / 2|, unit-modulus off-diagonals), whole and as a block shifted to be positive definite"""
    out = []
    for M, shift in ((N, 0.0), (N - 2, 1.25)):
        W = np.zeros((N, N), complex)
        W[np.arange(M), np.arange(M)] = np.abs(np.arange(M) - (M - 1) / 2.0) + shift
        ph = np.exp(1j * rng.uniform(-np.pi, np.pi, M - 1))
        W[np.arange(M - 1), np.arange(1, M)] = ph
        W[np.arange(1, M), np.arange(M - 1)] = ph.conj()
        out.append(W)
    return out


def _scaled(scale):
    def f(rng, N, thresh):
        out = []
        for k in range(4):
            X = rng.randn(N, 7) + 1j * rng.randn(N, 7)
            s = rng.randn(N) + 1j * rng.randn(N)
            X = X + 3.0 * k * np.outer(s, rng.randn(7) + 1j * rng.randn(7))
            out.append((X @ X.conj().T) * scale)
        return out
    return f


def _u0_zero(rng, N, thresh):
    """channel 0 decoupled from the rest: the top eigenvector (of the other N - 1 channels' block) has u_0 = 0 exactly"""
    out = []
    for _ in range(3):
        R = np.zeros((N, N), complex)
        R[0, 0] = 0.3
        R[1:, 1:] = _from_spectrum(rng, [1.0, 0.1] + _tail(rng, N - 1, 0.1, 2))
        out.append(R)
    return out


def _u0_tiny(rng, N, thresh):
    out = []
    for _ in range(3):
        q = rng.randn(N) + 1j * rng.randn(N)
        q[0] = 1e-9 * q[0] / abs(q[0])
        out.append(_from_spectrum(rng, [1.0, 0.1] + _tail(rng, N, 0.1, 2), first=q / np.linalg.norm(q)))
    return out


def _exact_tie(rng, N, thresh):
    """l1 = thresh * l2 with no rounding anywhere (diagonal input: no rotation runs, LAPACK returns the diagonal): '>' fails"""
    out = []
    for k in range(4):
        d = np.concatenate([[thresh, 1.0], rng.uniform(0.0, 0.8, N - 2)]) * 2.0 ** (3 * k)
        out.append(np.diag(d[rng.permutation(N)]).astype(complex))
    return out


MATRIX_FAMILIES = {
    'exact_tie': ('diagonal matrices with l1 = thresh * l2 exactly: the strict inequality decides', _exact_tie),
    'rank1': ('v v^H, random complex v', _rank1),
    'rank1_eps': ('unit v v^H + eps I, eps = 1e-16 .. 1e-2', _rank1_eps),
    'knife_edge': ('top pair at l1 / l2 = thresh (1 +- 2^-k), every k = 10 .. 50 (|m| > 1e-12 up to k = 39), random tail below', _knife_edge),
    'multiple_top': ('top eigenvalue exactly 2-, 3-, N/2- and N-fold', _multiple_top),
    'nm1_equal': ('N - 1 equal eigenvalues plus one, above or below them', _nm1_equal),
    'geometric12': ('geometric spectrum over 12 decades', _geometric(12)),
    'geometric30': ('geometric spectrum over 30 decades', _geometric(30)),
    'graded': ('D A D, A a random covariance, D = diag spanning 1e-4 .. 1 (ordered and shuffled)', _graded),
    'duplicated': ('covariance of data with two or three identical channels (duplicated rows and columns)', _duplicated),
    'zero': ('the zero matrix', _zero),
    'wilkinson': ('Hermitian Wilkinson tridiagonal W+, whole (indefinite) and as a positive definite block', _wilkinson),
    'scale_1e-24': ('random 7-snapshot covariances times 1e-24', _scaled(1e-24)),
    'scale_1e+12': ('random 7-snapshot covariances times 1e+12', _scaled(1e+12)),
    'u0_zero': ('top eigenvector with u_0 exactly 0 (channel 0 decoupled)', _u0_zero),
    'u0_tiny': ('top eigenvector with |u_0| = 1e-9', _u0_tiny),
}


def matrices(name, N, thresh, seed=0):
    """-> [m][n][n] complex128, n = N padded to even; exactly Hermitian"""
    idx = sorted(MATRIX_FAMILIES).index(name)
    rng = np.random.RandomState(100000 * seed + 1000 * idx + 10 * N + int(thresh))
    A = _herm(np.stack([np.asarray(a, complex) for a in MATRIX_FAMILIES[name][1](rng, N, thresh)]))
    assert np.array_equal(A, np.conj(np.swapaxes(A, -1, -2)))
    return embed(A)


# ---------------------------------------------------------------------------------------------------------------- audio
FS, N_SAMPLES = 24000, 24000 + 77          # 81 frames at hop 300; the last frame is not centred on the last sample
AUDIO_N_CH = (5, 6, 7, 8, 9, 10, 13, 16)
LEVEL = 0.1


def _source(rng, n, n_ch, step):
    """white source seen by n_ch microphones with an integer circular delay of `step` samples per microphone"""
    s = rng.randn(n)
    return np.stack([np.roll(s, c * step) for c in range(n_ch)])


def _two(rng, n, n_ch, a1=1.0, a2=1.0):
    return a1 * _source(rng, n, n_ch, 1) + a2 * _source(rng, n, n_ch, -2)


def _a_one_source(rng, n, C):
    return LEVEL * _source(rng, n, C, 1)


def _a_ramp(rng, n, C):
    ratio = 16.0 * (1.0 / 32.0) ** (np.arange(n) / (n - 1.0))        # P1 / P2: 16 -> 0.5, through 5, 4 and 1.05
    return LEVEL * (_source(rng, n, C, 1) + np.sqrt(1.0 / ratio)[None] * _source(rng, n, C, -2))


def _a_equal_power(rng, n, C):
    return LEVEL * _two(rng, n, C)


def _a_gains(rng, n, C):
    # amplitude 1 .. 1e-2, NOT 1 .. 1e-4: kappa_c grows as 1 / |u_c|, and with amplitudes down to 1e-4 a share of 1 / (C - 1) or more
    # of the elements would carry a bound above 1e-3 rad, against the 1 % the comparison rules allow to be left out
    g = np.logspace(0, -2, C)
    return LEVEL * g[:, None] * _two(rng, n, C, 1.0, 0.3)


def _a_twin(rng, n, C):
    y = LEVEL * _two(rng, n, C, 1.0, 0.3)
    y[2] = y[1]
    return y


def _a_silent_mid(rng, n, C):
    y = LEVEL * _two(rng, n, C, 1.0, 0.3)
    y[C // 2] = 0.0
    return y


def _a_silent_ch0(rng, n, C):
    y = LEVEL * _two(rng, n, C, 1.0, 0.3)
    y[0] = 0.0
    return y


def _a_silence_stretches(rng, n, C):
    y = LEVEL * _two(rng, n, C, 1.0, 0.3)
    y[:, 5000:9000] = 0.0                                            # 13 and 20 hops: longer than the 7-frame window
    y[:, 15000:21000] = 0.0
    return y


def _a_tiny(rng, n, C):
    return 1e-6 * _two(rng, n, C, 1.0, 0.3)


def _a_fail_then_pass(rng, n, C):
    env = np.where((np.arange(n) >= n // 3) & (np.arange(n) < 2 * n // 3), 1.0, 0.02)
    return LEVEL * (_source(rng, n, C, 1) + env[None] * _source(rng, n, C, -2))


AUDIO_FAMILIES = {
    'one_source': ('one delayed white source, no noise', _a_one_source),
    'ramp': ('two sources, power ratio ramping 16 -> 0.5 in time (through every threshold)', _a_ramp),
    'equal_power': ('two equal-power sources', _a_equal_power),
    'gains': ('two sources (10 dB apart), per-channel gains 1 .. 1e-2 in amplitude (1 .. 1e-4 in power)', _a_gains),
    'twin': ('two sources, channels 1 and 2 identical', _a_twin),
    'silent_mid': ('two sources, the middle channel silent', _a_silent_mid),
    'silent_ch0': ('two sources, channel 0 silent', _a_silent_ch0),
    'silence_stretches': ('two sources with two stretches of digital silence longer than the averaging window', _a_silence_stretches),
    'tiny': ('two sources at 1e-6 of full scale', _a_tiny),
    'fail_then_pass': ('one source; a second of equal power in the middle third only (gate fails there, passes again after)',
                       _a_fail_then_pass),
}


def audio(name, n_ch, seed=0, n=N_SAMPLES):
    idx = sorted(AUDIO_FAMILIES).index(name)
    rng = np.random.RandomState(7000000 + 100000 * seed + 1000 * idx + n_ch)
    return np.ascontiguousarray(AUDIO_FAMILIES[name][1](rng, n, n_ch), dtype=np.float32)


OPTIONS = tuple((thr, trk) for trk in (True, False) for thr in THRESHOLDS)     # 6 (ew_thresh, is_tracking) pairs


def audio_cases():
    """Every family at two microphone counts, three of the six (ew_thresh, is_tracking) pairs at each: every family meets tracking
    on and off and every threshold, every count of AUDIO_N_CH is met by at least two families.
    -> list of (family, n_ch, ew_thresh, is_tracking)"""
    out = []
    for i, name in enumerate(sorted(AUDIO_FAMILIES)):
        for j, n_ch in enumerate((AUDIO_N_CH[i % 8], AUDIO_N_CH[(i + 3) % 8])):
            for thr, trk in (OPTIONS[j::2] if i % 2 == 0 else OPTIONS[1 - j::2]):
                out.append((name, n_ch, thr, trk))
    return out
