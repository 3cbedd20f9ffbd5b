"""CPU side of the diffuse ambient noise (no GPU calls): the hash's statistics, the geometry and the expected
coherence of the three fields against closed forms and a dense quadrature, the composed torch path against the float64 reference of
tests/diffuse_reference.py, the level and SNR arithmetic, and the launcher's refusals.

Coherence bounds.  The reference is the closed form or the dense quadrature (diffuse_reference.dense_sphere, 8192 points), never the
field at another D.  Largest deviation over the 4 x 4 matrix and f = 100, 200 .. 4000 Hz, measured on a CPU (numpy float64; the
quantity is deterministic, the margin of 1.5 covers a change of the lattice's phase only):

    D     |sum u u^T / D - I / 3|   FOA off-diagonal   FOA X,Y,Z : W - 1/3   MIC open - sinc   MIC open - quadrature   MIC rigid - quadrature
    16    1.170696e-02              3.519073e-02       1.321989e-03          1.075345e-01      1.075345e-01            2.437332e-01
    32    4.365496e-03              1.310332e-02       3.480640e-04          2.214276e-02      2.214276e-02            4.035076e-02
    64    8.923447e-04              2.699178e-03       3.801117e-04          7.190913e-03      7.190913e-03            7.540590e-03
    128   5.031450e-04              1.509629e-03       8.592630e-05          1.464399e-03      1.464399e-03            2.292266e-03

(the FOA coherence's off-diagonal is the lattice's second moment over the geometric mean of two powers of about 1/3 and 1, or its first
moment: the same size as the first column; the quadrature agrees with sinc(2 pi f d / c) to 1e-14.)  The default D = 64 is asserted at
1.5 x its row, and no column may grow from D = 32 to D = 128."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import diffuse_reference as ref
from conftest import ROOT
from salsa_amd import ambient as amb
from salsa_amd import rooms
from salsa_amd import scenes as sc

MEASURED_D64 = dict(lattice=8.923447e-04, foa_off=2.699178e-03, foa_ratio=3.801117e-04, open_sinc=7.190913e-03, open_quad=7.190913e-03,
                    rigid_quad=7.540590e-03)
MARGIN = 1.5
FREQS = np.arange(100.0, 4001.0, 100.0)
FACTOR = 4.0                       # the bound of tests/test_attn_gpu.py's _holds: error <= 4 x the float32 evaluations' + one ulp


@pytest.fixture(scope='module')
def lib():
    from salsa_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------------------------------ white
N_STAT = 1 << 20


@pytest.fixture(scope='module')
def stretch():
    return ref.white(2021, 5, np.arange(N_STAT, dtype=np.int64)).astype(np.float64)


def test_white_has_mean_zero_and_variance_one(stretch):
    assert abs(stretch.mean()) <= 6.0 / np.sqrt(N_STAT)
    assert abs(stretch.var() - 1.0) <= 6.0 * np.sqrt(1.7 / N_STAT)            # kurtosis of Irwin-Hall-4 (2.7) minus 1


def test_white_is_uncorrelated_across_directions_seeds_and_lags(stretch):
    n = np.arange(N_STAT, dtype=np.int64)
    bound = 6.0 / np.sqrt(N_STAT)
    assert abs(np.mean(stretch * ref.white(2021, 6, n))) <= bound              # two directions
    assert abs(np.mean(stretch * ref.white(2022, 5, n))) <= bound              # two seeds (the default: consecutive ones)
    for lag in range(1, 65):
        assert abs(np.dot(stretch[:-lag], stretch[lag:]) / N_STAT) <= bound, lag


def test_white_is_defined_before_sample_zero_and_its_fields_take_both_extremes():
    n = np.arange(-ref.WHITE_LEAD, 64, dtype=np.int64)
    early = ref.white(7, 0, n)
    assert np.isfinite(early).all() and len(np.unique(early[:ref.WHITE_LEAD])) > 900
    assert np.array_equal(early[ref.WHITE_LEAD:], ref.white(7, 0, np.arange(64)))            # a sample's value does not depend on the stretch
    with pytest.raises(ValueError):
        ref.white_fields(7, 0, np.array([-ref.WHITE_LEAD - 1]))
    fields = ref.white_fields(2021, 5, np.arange(N_STAT, dtype=np.int64))
    assert fields.shape == (N_STAT, 4)
    assert np.all(fields.min(axis=0) == 0) and np.all(fields.max(axis=0) == 65535)
    lo, hi = np.float32(-131070) * ref.WHITE_SCALE, np.float32(131070) * ref.WHITE_SCALE     # the value's range: +- 2 sqrt(3) 65535 / 65536
    assert abs(float(hi) - 2.0 * np.sqrt(3.0 * 65535.0 / 65537.0)) < 1e-6 and lo == -hi


def test_torch_hash_equals_the_numpy_restatement_bit_for_bit():
    n = np.concatenate([np.arange(-1024, 2000), [2 ** 31 - 1, 2 ** 31, 2 ** 40 - 1, 2 ** 40 + 7]]).astype(np.int64)
    for seed in (0, 1, 2 ** 63, 2 ** 64 - 1, 0x123456789ABCDEF0):
        seeds = amb._seeds_on([seed], 1, 'cpu')
        for d in (0, 3, 255):
            got = amb.white(seeds, torch.tensor([d]), torch.from_numpy(n))[0, 0].numpy()
            assert np.array_equal(got, ref.white(seed, d, n)), (seed, d)
    assert amb.WHITE_SCALE == float(ref.WHITE_SCALE) and amb.WHITE_LEAD == ref.WHITE_LEAD


# --------------------------------------------------------------------------------------------------------------- field geometry
def _deviations(D):
    caps = sc.MIC_RADIUS * rooms._capsule_units()
    u, w = ref.dense_sphere()
    foa = amb.DiffuseField('foa', n_directions=D, colour='white')
    uu = foa.directions
    coh = foa.coherence([1000.0])[0]
    power = (np.abs(foa.response([1000.0])[0]) ** 2).sum(axis=0)
    dist = np.linalg.norm(caps[:, None] - caps[None], axis=-1)
    sinc = np.sinc(2.0 * FREQS[:, None, None] * dist[None] / sc.SOUND_SPEED)                  # sin(k d) / (k d)
    quad_open, _ = ref.coherence(ref.open_transfer(u, caps, FREQS, sc.SOUND_SPEED), w)
    cos_q = np.clip(u @ rooms._capsule_units().T, -1.0, 1.0)
    quad_rigid, _ = ref.coherence(rooms.sphere_response(FREQS[:, None, None], cos_q[None]), w)
    mic_open = amb.DiffuseField('mic', n_directions=D, colour='white').coherence(FREQS)
    mic_rigid = amb.DiffuseField('mic', baffle='rigid', n_directions=D, colour='white').coherence(FREQS)
    return dict(lattice=np.abs(uu.T @ uu / D - np.eye(3) / 3.0).max(), foa_off=np.abs(coh - np.eye(4)).max(),
                foa_ratio=np.abs(power[1:] / power[0] - 1.0 / 3.0).max(), open_sinc=np.abs(mic_open - sinc).max(),
                open_quad=np.abs(mic_open - quad_open).max(), rigid_quad=np.abs(mic_rigid - quad_rigid).max(),
                quad_check=np.abs(quad_open - sinc).max())


@pytest.fixture(scope='module')
def deviations():
    return {D: _deviations(D) for D in (32, 64, 128)}


def test_the_dense_quadrature_reproduces_the_closed_forms(deviations):
    assert deviations[64]['quad_check'] < 1e-12                               # open capsules: sinc(k d)
    coh, power = ref.coherence(ref.foa_transfer(ref.dense_sphere()[0]), ref.dense_sphere()[1])
    assert np.abs(coh - np.eye(4)).max() < 1e-12 and np.abs(power[0] - [1.0, 1 / 3, 1 / 3, 1 / 3]).max() < 1e-12     # 8192 terms


@pytest.mark.parametrize('what', sorted(MEASURED_D64))
def test_default_field_is_as_diffuse_as_measured_and_more_directions_do_not_hurt(deviations, what):
    print('DEVIATION %s: %s' % (what, {D: '%.6e' % deviations[D][what] for D in deviations}))
    assert deviations[64][what] <= MARGIN * MEASURED_D64[what]
    assert deviations[128][what] <= deviations[32][what]


def test_field_shapes_and_refusals():
    foa, mic, rigid = (amb.DiffuseField(f, baffle=b, n_directions=8, colour='white') for f, b in (('foa', 'open'), ('mic', 'open'), ('mic', 'rigid')))
    st = rooms.sphere_table()
    assert foa.mix.shape == (8, 4, 1) and mic.mix.shape == (8, 4, 39) and rigid.mix.shape == (8, 4, st.lead + st.trail + 1)
    assert all(f.mix.dtype == np.float32 and f.colour.dtype == np.float64 and f.directions.shape == (8, 3) for f in (foa, mic, rigid))
    assert np.allclose(np.linalg.norm(foa.directions, axis=1), 1.0, atol=1e-15)
    u = foa.directions
    assert np.array_equal(foa.mix[:, :, 0], np.stack([np.ones(8), u[:, 1], u[:, 2], u[:, 0]], axis=1).astype(np.float32))
    # the open capsules' taps are make_rir_bank's windowed sinc, three taps later (lead 19 against 16), and none of its support is cut
    assert np.abs(mic.mix.astype(np.float64).sum(axis=2) - 1.0).max() < 2e-3                 # a fractional delay has unit gain at 0 Hz
    assert np.all(mic.mix[:, :, 0] == 0) and np.all(mic.mix[:, :, -1] == 0)
    with pytest.raises(ValueError):
        amb.DiffuseField('foa', baffle='rigid')
    for bad in (dict(audio_format='wxyz'), dict(audio_format='mic', baffle='soft'), dict(audio_format='foa', n_directions=0),
                dict(audio_format='foa', n_directions=257), dict(audio_format='foa', colour='brown')):
        with pytest.raises(ValueError):
            amb.DiffuseField(**bad)
    assert sc.DiffuseField is amb.DiffuseField and sc.add_diffuse is amb.add_diffuse and sc.diffuse_noise is amb.diffuse_noise


def test_colours_have_unit_energy_linear_phase_and_the_stated_slopes():
    for name in ('white', 'pink', 'room'):
        g = amb.colour_filter(name)
        assert abs(np.sum(g * g) - 1.0) <= 1e-12, name
        assert len(g) % 2 == 1 and len(g) <= 513 and np.array_equal(g, g[::-1])
    assert np.array_equal(amb.colour_filter('white'), [1.0])
    f = np.array([500.0, 1000.0, 2000.0, 4000.0])
    for name, db_per_octave in (('pink', -10.0 * np.log10(2.0)), ('room', -5.0)):
        g = amb.colour_filter(name)
        mag = np.abs(np.exp(-2j * np.pi * f[:, None] * np.arange(len(g))[None] / sc.FS) @ g)
        assert np.abs(np.diff(20.0 * np.log10(mag)) - db_per_octave).max() < 0.1, name
    pair = amb.colour_filter(([0.0, 1000.0, 1100.0, 12000.0], [1.0, 1.0, 0.0, 0.0]), taps=257)
    assert len(pair) == 257 and abs(np.sum(pair * pair) - 1.0) <= 1e-12
    for bad in (([0.0, 0.0], [1.0, 1.0]), ([0.0, 1.0], [0.0, 0.0]), ([0.0, 1.0], [1.0])):
        with pytest.raises(ValueError):
            amb.colour_filter(bad)
    with pytest.raises(ValueError):
        amb.colour_filter('pink', taps=512)


# ------------------------------------------------------------------------------------------------------------------ torch path
def _holds(name, got, ref64, ref32):
    err = np.abs(np.asarray(got, np.float64) - ref64).max()
    yard = max(np.abs(r.astype(np.float64) - ref64).max() for r in ref32)
    floor = float(np.spacing(np.float32(np.abs(ref64).max())))
    print('RATIO %s err %.3e yard %.3e floor %.3e' % (name, err, yard, floor))
    assert err <= FACTOR * yard + floor, (name, err, yard, floor)


@pytest.mark.parametrize('fmt,colour,with_input', [('foa', 'room', True), ('foa', 'white', False), ('mic', 'pink', True), ('mic', 'room', False)])
def test_torch_path_equals_the_float64_reference(fmt, colour, with_input, monkeypatch):
    monkeypatch.setattr(amb, 'TORCH_CHUNK', 300)                               # three steps, the last a short one
    field = amb.DiffuseField(fmt, n_directions=5, colour=colour)
    N, seeds = 701, [11, 2 ** 64 - 3]
    x = torch.from_numpy(np.random.default_rng(3).standard_normal((2, 4, N)).astype(np.float32)) * 1e-3
    level = np.array([-60.0, -50.0])
    scales = field.scale_for(level).astype(np.float32)
    got = amb.add_diffuse(x.clone(), field, level_db=level, seeds=seeds) if with_input \
        else amb.diffuse_noise(field, 2, N, level_db=level, seeds=seeds, device='cpu')
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 4, N)
    for b in range(2):
        args = (field.mix, field.colour32, seeds[b], scales[b], N, x[b].numpy() if with_input else None)
        _holds('%s %s clip %d' % (fmt, colour, b), got[b].numpy(), ref.diffuse(*args),
               [ref.diffuse(*args, dtype=np.float32, reverse=r) for r in (False, True)])


def test_channel_power_is_the_references_expectation_and_a_long_render_has_it():
    for fmt, baffle, colour in (('foa', 'open', 'room'), ('mic', 'open', 'pink'), ('mic', 'rigid', 'white')):
        field = amb.DiffuseField(fmt, baffle=baffle, n_directions=16, colour=colour)
        want = ref.channel_power(field.mix, field.colour32)
        assert np.abs(field.channel_power / want - 1.0).max() < 1e-12
    field = amb.DiffuseField('foa', n_directions=16, colour='white')           # white: every sample is independent, var(x^2) <= 3 P^2
    assert np.allclose(field.channel_power, [16.0, 16.0 / 3, 16.0 / 3, 16.0 / 3], rtol=0.05)
    N = 1 << 16
    y = amb.diffuse_noise(field, 1, N, level_db=0.0, seeds=5, device='cpu')[0].double().numpy()
    got = (y ** 2).mean(axis=1) / float(field.scale_for(0.0)) ** 2
    assert np.abs(got / field.channel_power - 1.0).max() <= 6.0 * np.sqrt(2.0 / N)


# ----------------------------------------------------------------------------------------------------------------------- levels
def _power_estimator_sigma(field, N):
    """Relative standard deviation of the estimator P^ = sum_c sum_n x_c[n]^2 / (4 N) of a rendered clip's mean square, in float64.
    x is a sum of many independent terms, so its fourth moments are taken as Gaussian: cov(x_i[n]^2, x_j[n']^2) = 2 R_ij(n - n')^2,
    var(P^) = 2 / (4 N)^2 sum_ij sum_tau (N - |tau|) R_ij(tau)^2.  R_ij is the inverse transform of the cross spectrum S_ij(f) = sum_d
    F_di conj(F_dj) |G(f)|^2: what .coherence normalises, times the powers it divides by and the colour's spectrum (whose inverse
    transform is the colour's autocorrelation).  The support of R is below La + Lg taps, far inside the 4096-point transform."""
    nfft = 4096
    f = np.fft.rfftfreq(nfft, 1.0 / field.fs)
    F = field.response(f)
    coh = field.coherence(f)
    p = np.real(np.einsum('fdc,fdc->fc', F, np.conj(F)))
    G2 = np.abs(np.fft.rfft(field.colour32.astype(np.float64), nfft)) ** 2                    # the colour's autocorrelation, transformed
    S = coh * np.sqrt(p[:, :, None] * p[:, None, :]) * G2[:, None, None]
    R = np.fft.irfft(S, nfft, axis=0)                                                         # R[tau mod nfft, i, j]
    tau = np.minimum(np.arange(nfft), nfft - np.arange(nfft))
    var = 2.0 / (4.0 * N) ** 2 * np.sum((N - tau)[:, None, None] * R ** 2)
    mean = np.trace(R[0]) / 4.0
    assert abs(mean / field.channel_power.mean() - 1.0) < 1e-9
    return np.sqrt(var) / mean


@pytest.mark.parametrize('fmt,colour', [('foa', 'room'), ('mic', 'pink')])
def test_add_diffuse_realises_the_snr(fmt, colour):
    field = amb.DiffuseField(fmt, n_directions=16, colour=colour)
    N, snr = 2 * sc.FS, np.array([20.0, 5.0, 10.0])
    t = np.arange(N) / sc.FS
    audio = np.zeros((3, 4, N), np.float32)
    audio[0] = 0.2 * np.sin(2 * np.pi * 440.0 * t)[None] * np.array([1.0, 0.5, -0.5, 0.25])[:, None]
    audio[1] = 0.01 * np.random.default_rng(0).standard_normal((4, N))
    x = torch.from_numpy(audio)                                                # clip 2 is silent
    out = amb.add_diffuse(x.clone(), field, snr_db=snr, seeds=100)
    assert np.array_equal(out[2].numpy().view(np.uint32), audio[2].view(np.uint32))          # a silent clip keeps its bits
    sigma = _power_estimator_sigma(field, N)
    print('SIGMA %s %s: %.4f' % (fmt, colour, sigma))
    assert 0.001 < sigma < 0.2
    for b in range(2):
        signal = np.mean(audio[b].astype(np.float64) ** 2)
        noise = np.mean((out[b].numpy().astype(np.float64) - audio[b]) ** 2)
        expected = signal / 10.0 ** (snr[b] / 10.0)
        # the sum's rounding moves a noise sample by at most half an ulp of the output: a relative 2^-23 sqrt(signal / noise) on the power
        slack = 2.0 ** -23 * np.sqrt(np.max(np.abs(out[b].numpy())) ** 2 / expected)
        print('SNR clip %d: asked %.1f dB, realised %.3f dB, 6 sigma = %.3f' % (b, snr[b], 10 * np.log10(signal / noise), 6 * sigma))
        assert abs(noise / expected - 1.0) <= 6.0 * sigma + slack, b
    again = amb.add_diffuse(x.clone(), field, snr_db=snr, seeds=100)
    assert torch.equal(out, again)
    other = amb.add_diffuse(x.clone(), field, snr_db=snr, seeds=101)
    assert not torch.equal(out[0], other[0]) and torch.equal(other[0], amb.add_diffuse(x[:1].clone(), field, snr_db=20.0, seeds=[101])[0])


def test_level_arguments():
    field = amb.DiffuseField('foa', n_directions=4, colour='white')
    x = torch.zeros(1, 4, 64)
    for kw in (dict(), dict(snr_db=10.0, level_db=-40.0)):
        with pytest.raises(ValueError):
            amb.add_diffuse(x.clone(), field, **kw)
    y = amb.add_diffuse(x, field, level_db=-40.0)
    assert y is x and float(x.abs().max()) > 0                                 # without `out` the sum lands in the audio itself
    z = torch.zeros(1, 4, 64)
    w = amb.add_diffuse(z, field, level_db=-40.0, out=torch.empty(1, 4, 64))
    assert float(z.abs().max()) == 0 and torch.equal(w, x)
    assert abs(float(field.scale_for(-40.0)) ** 2 * field.channel_power.mean() - 1e-4) < 1e-18
    assert torch.equal(amb.diffuse_noise(field, 2, 64, seeds=None, device='cpu'), amb.diffuse_noise(field, 2, 64, seeds=[0, 1], device='cpu'))
    assert torch.equal(amb.diffuse_noise(field, 2, 64, seeds=9, device='cpu')[1], amb.diffuse_noise(field, 1, 64, seeds=[10], device='cpu')[0])
    with pytest.raises(ValueError):
        amb.diffuse_noise(field, 2, 64, seeds=[1, 2, 3], device='cpu')
    with pytest.raises(ValueError):
        amb.add_diffuse(torch.zeros(1, 3, 64), field, level_db=-40.0)


# -------------------------------------------------------------------------------------------------------------------- refusals
P = C.c_void_p(0x1000)          # stands in for a pointer: every call below is refused before anything reads it or touches a device
S = None                        # the null stream


def test_launcher_refuses_shapes_one_step_outside_and_null_pointers(lib):
    from salsa_amd import _lib
    assert lib.salsa_scene_diffuse_block() == 2048
    sup = lib.salsa_scene_diffuse_supported
    assert sup(4, 1, 1, 1) == 1 and sup(4, 256, 128, 513) == 1 and sup(4, 64, 39, 257) == 1
    bad_shapes = [(3, 64, 32, 513), (5, 64, 32, 513), (4, 0, 32, 513), (4, 257, 32, 513), (4, 64, 0, 513), (4, 64, 129, 513), (4, 64, 32, 0),
                  (4, 64, 32, -1), (4, 64, 32, 515), (4, 64, 32, 512), (4, 64, 32, 2)]
    for shape in bad_shapes:
        assert sup(*shape) == 0, shape
    # mix, D, C, La, colour, Lg, seeds, scales, in, out, clips, samples, stream
    ok = [P, 64, 4, 32, P, 513, P, P, P, P, 3, 48000, S]
    for i in (0, 4, 6, 7, 9):                                                  # d_in (8) may be null
        rc = lib.salsa_scene_diffuse(*[None if k == i else a for k, a in enumerate(ok)])
        assert rc == _lib.E_INVAL and b'salsa_scene_diffuse' in lib.salsa_last_error(), i
    for Cn, D, La, Lg in bad_shapes:
        assert lib.salsa_scene_diffuse(P, D, Cn, La, P, Lg, P, P, None, P, 3, 48000, S) == _lib.E_INVAL, (Cn, D, La, Lg)
    for clips, samples in ((0, 48000), (-1, 48000), (3, 0), (3, -1), (3, 1 << 32), (2048, (1 << 32) - 1)):     # the last: 2^32 blocks
        assert lib.salsa_scene_diffuse(P, 64, 4, 32, P, 513, P, P, None, P, clips, samples, S) == _lib.E_INVAL, (clips, samples)


# ------------------------------------------------------------------------------------------------------ the training tool's draw
def _tool():
    spec = importlib.util.spec_from_file_location('train_on_scenes', os.path.join(ROOT, 'tools', 'train_on_scenes.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_on_scenes_default_ambient_is_the_white_draw_number_for_number():
    tool = _tool()
    args = tool.parse_args([])
    assert args.ambient == 'white' and args.snr_db == 20.0
    g = torch.Generator('cpu').manual_seed(2021)
    first, diffuse = tool.scene_ambient(args, None, 3, 500, 'cpu', g, 0)
    second, _ = tool.scene_ambient(args, None, 2, 500, 'cpu', g, 0)
    g = torch.Generator('cpu').manual_seed(2021)                               # the lines the tool ran before it had the option
    assert diffuse is None
    assert torch.equal(first, 1e-3 * torch.randn(3, 4, 500, device='cpu', generator=g))
    assert torch.equal(second, 1e-3 * torch.randn(2, 4, 500, device='cpu', generator=g))
    args = tool.parse_args(['--ambient', 'diffuse', '--snr-db', '15', '--format', 'mic', '--baffle', 'rigid'])
    field = object()
    g = torch.Generator('cpu').manual_seed(1)
    state = g.get_state()
    assert tool.scene_ambient(args, field, 3, 500, 'cpu', g, 77) == (None, (field, dict(snr_db=15.0, seed=77)))
    assert torch.equal(g.get_state(), state)                                   # ... and draws nothing
