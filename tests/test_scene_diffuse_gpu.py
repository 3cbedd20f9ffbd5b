"""The diffuse ambient noise on the GPU: salsa_scene_diffuse through the C ABI, every output between NaN guard
bands, against the float64 reference of tests/diffuse_reference.py; the hash's bits; the structural promises; the composed torch path
on the device; and add_scenes(diffuse=...) end to end.

Bound of every comparison with float64, the project's existing one (test_attn_gpu._holds): the kernel's maximum error may be at most 4
times the largest error of the FLOAT32 evaluations of the same reference on that case (natural order, and d, k and j all reversed),
plus one float32 ulp of the tensor's largest magnitude.  Shapes: the smallest at which the kernel can go wrong.  With BLOCK = 2048 the
kernel's output block, N in {1, BLOCK - 1, BLOCK, BLOCK + 1, 2 BLOCK + 17}; D in {1, 3, 64}; (La, Lg) in {(1, 1), (1, 513), (32, 1),
(32, 257), (128, 513)} and the rigid table's La = 80 (with the 'room' colour, 513 taps); B in {1, 3}.  Every N meets every (La, Lg) at D =
3; D = 1 and D = 64 meet the extreme and a middle (La, Lg) at the N that has a whole, a second and a partial block."""
import functools

import numpy as np
import pytest
import torch

import diffuse_reference as ref
from salsa_amd import _lib
from salsa_amd import ambient as amb
from salsa_amd import scenes as sc
from test_attn_gpu import DEV, _check_guards, _guarded, _holds, _ptr, _stream

pytestmark = pytest.mark.gpu

BLOCK = 2048
SIZES = (1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 17)
TAPS = ((1, 1), (1, 513), (32, 1), (32, 257), (128, 513), ('rigid', 513))
MEASURED = """largest ratio (kernel error) / (largest float32-reference error) over the cases of a row, on one MI355X (0.00: the kernel's
error was zero; `-`: so was the yardstick), with the case that gave it:
  (La, Lg)       over every D, B and N of the two bound tests
  (1, 1)         2.28   (D 3, N 1: four numbers, error 4.1e-9 against a yardstick of 1.8e-9 and a one-ulp floor of 3.7e-9)
  (1, 513)       0.94   (D 3, N 2048)
  (32, 1)        1.00   (D 3, N 1)
  (32, 257)      1.07   (D 1, N 4113, B 3)
  (128, 513)     0.97   (D 64, N 4113)
  (rigid 80, 513) 0.96  (D 3, N 2049, B 3)
  add_diffuse on the device against the same reference: hip leg 1.00 (foa), 0.96 (mic open), 1.00 (mic rigid); torch leg 0.56, 0.88, 0.63;
  the two legs at most 2.6e-8 apart on outputs of magnitude 0.2.
(The kernel's fmaf chain in the definition's order is the float32 reference's natural order but for the fused rounding, hence ratios
near one.)"""


@pytest.fixture(scope='module')
def L():
    lib = _lib.load()
    assert lib.salsa_scene_diffuse_block() == BLOCK
    return lib


@functools.lru_cache(maxsize=None)
def _filters(D, La, Lg):
    """(mix (D, 4, La), colour (Lg,)) float32: the rigid field's own, or seeded random ones of the power a field has"""
    if La == 'rigid':
        field = amb.DiffuseField('mic', baffle='rigid', n_directions=D, colour='room')
        assert field.colour_taps == Lg
        return field.mix, field.colour32
    r = np.random.default_rng([D, La, Lg])
    mix = (r.standard_normal((D, 4, La)) / np.sqrt(La)).astype(np.float32)
    if La == 1:
        mix[0, 0, 0] = 1.0
    colour = r.standard_normal(Lg)
    return mix, (colour / np.sqrt(np.sum(colour ** 2))).astype(np.float32)


def _inputs(B, N, with_in):
    r = np.random.default_rng([B, N])
    seeds = [int(s) for s in r.integers(0, 2 ** 63, B)]
    seeds[-1] = 2 ** 64 - 1 - B
    scales = (10.0 ** r.uniform(-3.0, -1.0, B)).astype(np.float32)
    inp = (r.standard_normal((B, 4, N)) * 1e-2).astype(np.float32) if with_in else None
    return seeds, scales, inp


@functools.lru_cache(maxsize=None)
def _references(D, La, Lg, B, N, with_in):
    """float64, [float32 natural, float32 reversed], each (B, 4, N): computed once per case and shared"""
    mix, colour = _filters(D, La, Lg)
    seeds, scales, inp = _inputs(B, N, with_in)
    one = lambda b, **kw: ref.diffuse(mix, colour, seeds[b], scales[b], N, None if inp is None else inp[b], **kw)
    return (np.stack([one(b) for b in range(B)]),
            [np.stack([one(b, dtype=np.float32, reverse=rv) for b in range(B)]) for rv in (False, True)])


def _seed_tensor(seeds):
    return torch.from_numpy(np.array([s % (1 << 64) for s in seeds], np.uint64).view(np.int64)).to(DEV)


def _run(L, mix, colour, seeds, scales, inp, N, in_place=False):
    """one call through the C ABI -> float32 numpy (B, 4, N); the output (and an out-of-place input) lie between NaN guard bands"""
    B = len(seeds)
    d_mix, d_colour = torch.from_numpy(np.ascontiguousarray(mix)).to(DEV), torch.from_numpy(np.ascontiguousarray(colour)).to(DEV)
    d_seeds, d_scales = _seed_tensor(seeds), torch.from_numpy(np.asarray(scales, np.float32)).to(DEV)
    out_buf, out = _guarded((B, 4, N))
    d_in = None
    if inp is not None:
        if in_place:
            out.copy_(torch.from_numpy(inp))
            d_in = out
        else:
            d_in = torch.from_numpy(inp).to(DEV)
    rc = L.salsa_scene_diffuse(_ptr(d_mix), mix.shape[0], 4, mix.shape[2], _ptr(d_colour), len(colour), _ptr(d_seeds), _ptr(d_scales),
                               _ptr(d_in) if d_in is not None else None, _ptr(out), B, N, _stream())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    _check_guards((out_buf, out))
    if d_in is not None and not in_place:
        assert np.array_equal(d_in.cpu().numpy().view(np.uint32), inp.view(np.uint32)), 'the input was written'
    return out.cpu().numpy()


def _case(L, D, La, Lg, B, N, with_in):
    mix, colour = _filters(D, La, Lg)
    seeds, scales, inp = _inputs(B, N, with_in)
    return _run(L, mix, colour, seeds, scales, inp, N)


# ---- bound ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('La,Lg', TAPS)
@pytest.mark.parametrize('N', SIZES)
def test_every_block_edge_meets_every_filter_length(L, N, La, Lg):
    B = 3 if N == BLOCK + 1 else 1                                             # clips with an input at one size, noise alone at the others
    got = _case(L, 3, La, Lg, B, N, B == 3)
    ref64, ref32 = _references(3, La, Lg, B, N, B == 3)
    _holds('out', got, ref64, ref32, 'D 3 La %s Lg %d B %d N %d' % (La, Lg, B, N))


@pytest.mark.parametrize('D,La,Lg,B', [(1, 1, 1, 3), (1, 128, 513, 1), (1, 32, 257, 3), (64, 1, 1, 1), (64, 1, 513, 3), (64, 32, 257, 1),
                                       (64, 128, 513, 1), (64, 'rigid', 513, 1)])
def test_one_and_many_directions(L, D, La, Lg, B):
    N = 2 * BLOCK + 17
    got = _case(L, D, La, Lg, B, N, B == 3)
    ref64, ref32 = _references(D, La, Lg, B, N, B == 3)
    _holds('out', got, ref64, ref32, 'D %d La %s Lg %d B %d N %d' % (D, La, Lg, B, N))


# ---- bits -------------------------------------------------------------------------------------------------------------------------
def test_the_hash_on_the_device_is_the_numpy_restatement_bit_for_bit(L):
    """D = 1, the FOA gains (W's is 1) and colour = delta: W is scale x white, one rounded product; the lattice's one direction is +x,
    so Y and Z (gain 0) are zeros and X is W"""
    field = amb.DiffuseField('foa', n_directions=1, colour='white')
    assert field.mix.shape == (1, 4, 1) and field.mix[0, 0, 0] == 1.0 and np.array_equal(field.colour32, [1.0])
    N = 2 * BLOCK + 17
    seeds, scales = [0, 2 ** 64 - 1, 0x123456789ABCDEF0], np.array([1.0, 0.37, 1e-3], np.float32)
    got = _run(L, field.mix, field.colour32, seeds, scales, None, N)
    for b in range(3):
        want = scales[b] * ref.white(seeds[b], 0, np.arange(N, dtype=np.int64))
        assert want.dtype == np.float32 and np.array_equal(got[b, 0].view(np.uint32), want.view(np.uint32)), b
        for c, g in ((1, field.mix[0, 1, 0]), (2, field.mix[0, 2, 0]), (3, field.mix[0, 3, 0])):
            want_c = scales[b] * (g * ref.white(seeds[b], 0, np.arange(N, dtype=np.int64)) + np.float32(0.0))    # a chain starts at +0.0
            assert np.array_equal(got[b, c].view(np.uint32), want_c.view(np.uint32)), (b, c)


# ---- structure --------------------------------------------------------------------------------------------------------------------
D_S, LA_S, LG_S, N_S = 3, 32, 257, 2 * BLOCK + 17


@pytest.fixture(scope='module')
def batch(L):
    mix, colour = _filters(D_S, LA_S, LG_S)
    seeds, scales, inp = _inputs(3, N_S, True)
    return mix, colour, seeds, scales, inp, _run(L, mix, colour, seeds, scales, inp, N_S)


def _same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_two_runs_are_bit_equal_and_in_place_equals_out_of_place(L, batch):
    mix, colour, seeds, scales, inp, out = batch
    assert _same(_run(L, mix, colour, seeds, scales, inp, N_S), out)
    assert _same(_run(L, mix, colour, seeds, scales, inp, N_S, in_place=True), out)


def test_a_clip_does_not_depend_on_its_batch_or_its_place_in_it(L, batch):
    mix, colour, seeds, scales, inp, out = batch
    for b in range(3):
        assert _same(_run(L, mix, colour, seeds[b:b + 1], scales[b:b + 1], inp[b:b + 1], N_S)[0], out[b]), b
    order = [2, 0, 1]
    moved = _run(L, mix, colour, [seeds[i] for i in order], scales[order], np.ascontiguousarray(inp[order]), N_S)
    assert _same(moved, np.ascontiguousarray(out[order]))


@pytest.mark.parametrize('short', [1, 100, BLOCK - 1, BLOCK, BLOCK + 1])
def test_a_shorter_render_is_the_first_samples(L, batch, short):
    mix, colour, seeds, scales, inp, out = batch
    got = _run(L, mix, colour, seeds, scales, np.ascontiguousarray(inp[:, :, :short]), short)
    assert _same(got, np.ascontiguousarray(out[:, :, :short]))


def test_scale_zero_leaves_the_input_and_different_seeds_differ(L, batch):
    mix, colour, seeds, scales, inp, out = batch
    quiet = scales.copy()
    quiet[1] = 0.0
    inp = inp.copy()
    inp[1, 0, :5] = [-0.0, 0.0, np.float32(1e-45), -1.0, np.float32(3e38)]     # bits that an addition of 0 would not all keep
    for in_place in (False, True):
        got = _run(L, mix, colour, seeds, quiet, inp, N_S, in_place=in_place)
        assert _same(got[1], inp[1]) and _same(got[0], out[0]) and _same(got[2], out[2])
    alone = _run(L, mix, colour, seeds, np.array([0.0, -0.0, 0.0], np.float32), None, N_S)
    assert not alone.view(np.uint32).any()                                     # +0.0 without an input
    other = _run(L, mix, colour, [seeds[0] + 1, seeds[1], seeds[2]], scales, inp, N_S)
    assert not _same(other[0], out[0]) and np.abs(other[0] - out[0]).max() > 1e-4 and _same(other[2], out[2])


# ---- the torch path on the device, and end to end -----------------------------------------------------------------------------------
@pytest.mark.parametrize('fmt,baffle', [('foa', 'open'), ('mic', 'open'), ('mic', 'rigid')])
def test_hip_call_and_composed_torch_path_agree(fmt, baffle, monkeypatch):
    """both legs of add_diffuse on the device, at scales from snr_db computed there: each within the bound of the float64 reference at
    the scales they shared, hence within twice the bound of each other"""
    field = amb.DiffuseField(fmt, baffle=baffle, n_directions=5, colour='pink')
    N, seeds = BLOCK + 300, [3, 2 ** 64 - 9]
    x = (np.random.default_rng(8).standard_normal((2, 4, N)) * 0.05).astype(np.float32)
    x[1] *= 0.01
    audio = torch.from_numpy(x).to(DEV)
    monkeypatch.setattr(amb, 'TORCH_CHUNK', 1000)
    got = {}
    for leg, hip in (('hip', True), ('torch', False)):
        monkeypatch.setattr(sc, 'HIP_SCENE', hip)
        got[leg] = amb.add_diffuse(audio, field, snr_db=[20.0, 0.0], seeds=seeds, out=torch.empty_like(audio)).cpu().numpy()
    power = (x.astype(np.float64) ** 2).mean(axis=(1, 2))
    scales = np.sqrt(power / (10.0 ** (np.array([20.0, 0.0]) / 10.0) * field.channel_power.mean())).astype(np.float32)
    ref64 = np.stack([ref.diffuse(field.mix, field.colour32, seeds[b], scales[b], N, x[b]) for b in range(2)])
    ref32 = [np.stack([ref.diffuse(field.mix, field.colour32, seeds[b], scales[b], N, x[b], np.float32, rv) for b in range(2)]) for rv in (False, True)]
    for leg in got:
        print('LEG %s %s %s: the other leg is %.3e away' % (fmt, baffle, leg, np.abs(got['hip'] - got['torch']).max()))
        _holds(leg, got[leg], ref64, ref32, '%s %s' % (fmt, baffle))


def test_add_scenes_with_a_diffuse_field_fills_a_bank():
    from salsa_amd.dataset import GpuFeatureBank
    from salsa_amd.extractor import SalsaExtractor
    NC, n = 12, 2 * sc.FS
    pool = sc.synth_event_pool(NC, 2, 1, min_s=0.3, max_s=0.8)
    rbank = sc.make_rir_bank('foa', [(a, e) for a in range(-170, 180, 60) for e in (-30, 10)], 600, rt60=0.2, seed=2)
    scenes = sc.draw_scenes(2, pool, rbank, n, 4, gap_s=(0.1, 0.4))
    assert scenes.n_items >= 2
    field = sc.DiffuseField('foa', n_directions=16)
    ex = SalsaExtractor(audio_format='foa', fmax_doa=9000, device=torch.device(DEV))
    bank = GpuFeatureBank(ex, n_classes=NC, chunk_len_s=2.0, max_clip_s=2)
    audio = sc.add_scenes(bank, scenes, pool, rbank, diffuse=(field, dict(level_db=-45.0, seed=77)))
    assert tuple(audio.shape) == (2, 4, n) and bank.names == ['scene_0000', 'scene_0001'] and bank.clip_len == [160, 160]
    bank.fit_scaler()
    bank.finalize()
    assert len(bank) >= 2
    clean = sc.render_scenes(scenes, pool, rbank).cpu().numpy().astype(np.float64)
    noise = sc.diffuse_noise(field, 2, n, level_db=-45.0, seeds=77, device=DEV).cpu().numpy().astype(np.float64)
    got = audio.cpu().numpy()
    ulp = float(np.spacing(np.float32(np.abs(got).max())))
    assert np.abs(got - clean - noise).max() <= ulp
    with pytest.raises(ValueError):
        sc.add_scenes(bank, scenes, pool, rbank, diffuse=(sc.DiffuseField('mic', n_directions=4), dict(level_db=-45.0)))
    with pytest.raises(ValueError):
        sc.add_scenes(bank, scenes, pool, rbank, diffuse=(field, dict(level_db=-45.0, snr_db=10.0)))
