"""CPU tests of test-time chunks (reference data.test_chunk_len_s / test_chunk_hop_len_s) and of the host side of the device
decoding: infer_pipelined with chunks against a direct restatement, fixture g28 (tools/make_golden_test_chunks.py) through the host
functions, the chunk split, the YAML keys in frames, the per-element arithmetic of salsa_nn_seld_decode (salsa_amd/csrc/
seld_decode.h built with g++: tests/hostemu/decode_emu.cpp) against numpy, the export and the launcher's argument checks.

Angles follow one rule everywhere (KNIFE EDGES): the kernel computes them in float64, numpy's reference expression in float32, whose
largest deviation from float64 was measured at 2.6e-5 degrees over 4e6 tanh(N(0, 1)) triples; so azimuth and elevation must be EQUAL
wherever the float64 angle is more than 1e-4 degrees (four times that) from a half-integer, may differ by 1 inside that band (179
and -180 are adjacent), and at most 0.1 % of a test's active pairs may lie in the band (measured: 0.04 %) -- asserted before the
allowance is used."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

BAND_DEG, BAND_CAP = 1e-4, 1e-3


def angles64(x, y, z):
    x, y, z = (np.asarray(a, dtype=np.float64) for a in (x, y, z))
    return np.arctan2(y, x) * 180.0 / np.pi, np.arctan2(z, np.sqrt(x ** 2 + y ** 2)) * 180.0 / np.pi


def in_band(a):
    return np.abs((a - np.floor(a)) - 0.5) <= BAND_DEG


def assert_angles(got, want, exact64, what):
    """got / want (n,) integer degrees, exact64 the float64 angle: the knife-edge rule of the module docstring"""
    band = in_band(exact64)
    share = float(band.mean()) if band.size else 0.0
    assert share <= BAND_CAP, '%s: %.3f %% of the pairs lie in the rounding band' % (what, 100 * share)
    got, want = np.asarray(got, dtype=np.int64), np.asarray(want, dtype=np.int64)
    diff = np.abs(got - want)
    diff = np.minimum(diff, 360 - diff)                                  # 179 and -180 are one degree apart
    assert not diff[~band].any(), '%s: %d angles differ outside the band' % (what, int((diff[~band] != 0).sum()))
    assert diff.max(initial=0) <= 1, what


def g28_inputs(case, logit_mean):
    """the seeded inputs of one g28 case, drawn as tools/make_golden_test_chunks.py draws them"""
    g = torch.Generator().manual_seed(case['seed'])
    logit = torch.randn(case['n_chunks'], case['chunk_len'], case['n_classes'], generator=g) + logit_mean
    xyz = torch.tanh(torch.randn(case['n_chunks'], case['chunk_len'], 3 * case['n_classes'], generator=g))
    return torch.sigmoid(logit).numpy(), xyz.numpy()


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('decode_emu') / 'libdecode_emu.so')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-o', so,
                           os.path.join(ROOT, 'tests', 'hostemu', 'decode_emu.cpp')])
    L = C.CDLL(so)
    fp, sp = C.POINTER(C.c_float), C.POINTER(C.c_int16)
    L.emu_combine_step.restype = C.c_float
    L.emu_combine_step.argtypes = [C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int]
    L.emu_combine.argtypes = [fp] + [C.c_int] * 6 + [fp]
    L.emu_angles.argtypes = [fp, C.c_long, sp, sp]
    L.emu_decode.argtypes = [fp, fp] + [C.c_int] * 5 + [C.c_float, C.c_int, sp]
    return L


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _sp(a):
    return a.ctypes.data_as(C.POINTER(C.c_int16))


def emu_combine(emu, chunks, chunk_len, hop, n_frames, method):
    chunks = np.ascontiguousarray(chunks, dtype=np.float32)
    out = np.full((n_frames, chunks.shape[2]), np.nan, dtype=np.float32)
    emu.emu_combine(_fp(chunks), chunks.shape[0], chunk_len, hop, n_frames, chunks.shape[2], int(method == 'gmean'), _fp(out))
    return out


# ---------------------------------------------------------------------------------------------------- infer_pipelined
def toy_forward(seen=None, positive=False):
    """a deterministic CPU 'model': label frame j of a chunk reads feature frame 8 j of channel 0, bin 0 (pure indexing and
    element-wise arithmetic: a chunk's output does not depend on what else is in the batch); positive: directions in the first
    octant, which is where the geometric mean of chunks is a number"""
    w = torch.linspace(-1.0, 1.0, 12)
    v = torch.linspace(-2.0, 2.0, 36)

    def forward(x):
        if seen is not None:
            seen.append(x.shape[0])
        p = x[:, 0, ::8, 0][..., None]
        return torch.sigmoid(3.0 * p * w - 1.0), (lambda d: d.abs() if positive else d)(torch.tanh(p * v + 0.1 * v))
    return forward


@pytest.mark.parametrize('method,version', [('mean', '2021'), ('gmean', '2020')])
def test_infer_pipelined_with_chunks_equals_the_restatement(method, version):
    from salsa_amd.crnn.infer import infer_pipelined
    from salsa_amd.crnn.postprocess import combine_chunks, to_dcase_rows
    from salsa_amd.dataset import get_segment_idxes
    feats = torch.randn(5, 2, 960, 3, generator=torch.Generator().manual_seed(5))
    seen = []
    rows = infer_pipelined(5, lambda lo, hi: feats[lo:hi], toy_forward(seen, method == 'gmean'), sub_batch=2, depth=2, sed_threshold=0.4,
                           n_label_frames=120, chunk_len=320, chunk_hop_len=200, decode='host', combine_method=method,
                           eval_version=version)
    starts, _ = get_segment_idxes(960, 320, 200, 1, 0)
    assert starts == [0, 200, 400, 600, 640]
    assert seen == [6, 4, 6, 4, 5]                       # chunk_batch = 2 * 960 // 320 chunks per forward; the last sub-batch is partial
    fwd, n = toy_forward(None, method == 'gmean'), 0
    for i in range(5):
        p, d = fwd(torch.stack([feats[i, :, s:s + 320] for s in starts]))
        want = to_dcase_rows(combine_chunks(p.numpy(), 40, 25, n_frames=120, combine_method=method),
                             combine_chunks(d.numpy(), 40, 25, n_frames=120, combine_method=method), sed_threshold=0.4,
                             max_nframes_per_file=120, eval_version=version)
        assert rows[i] == want, i
        n += len(want)
    assert n > 100 and len(rows[0][0]) == (5 if version == '2021' else 4)
    seen.clear()
    again = infer_pipelined(5, lambda lo, hi: feats[lo:hi], toy_forward(seen, method == 'gmean'), sub_batch=2, depth=2, sed_threshold=0.4,
                            n_label_frames=120, chunk_len=320, chunk_hop_len=200, combine_method=method, eval_version=version,
                            chunk_batch=3)
    assert again == rows and seen == [3, 3, 3, 1] * 2 + [3, 2]


def test_infer_pipelined_whole_clip_through_the_chunk_keys_is_the_default_path():
    """seld.yml's setting (test_chunk_len_s 60.0, hop 60.1: a hop beyond the chunk) gives one chunk per clip and the rows the
    call without chunk keywords gives"""
    from salsa_amd.crnn.infer import infer_pipelined
    feats = torch.randn(3, 2, 960, 3, generator=torch.Generator().manual_seed(6))
    kw = dict(sub_batch=2, sed_threshold=0.4, n_label_frames=120)
    plain = infer_pipelined(3, lambda lo, hi: feats[lo:hi], toy_forward(), **kw)
    assert infer_pipelined(3, lambda lo, hi: feats[lo:hi], toy_forward(), chunk_len=960, chunk_hop_len=962, **kw) == plain
    assert sum(len(r) for r in plain) > 100


def test_infer_pipelined_refuses_what_it_cannot_combine():
    from salsa_amd.crnn.infer import infer_pipelined
    feats = torch.randn(2, 2, 960, 3, generator=torch.Generator().manual_seed(7))
    kw = dict(sub_batch=2, n_label_frames=120)
    with pytest.raises(ValueError, match='chunk_hop_len 400 > chunk_len 320'):
        infer_pipelined(2, lambda lo, hi: feats[lo:hi], toy_forward(), chunk_len=320, chunk_hop_len=400, **kw)

    def short(x):                                        # one label frame too few per chunk
        p, d = toy_forward()(x)
        return p[:, :-1], d[:, :-1]
    with pytest.raises(ValueError, match='gave 39 label frames .* expected 40'):
        infer_pipelined(2, lambda lo, hi: feats[lo:hi], short, chunk_len=320, chunk_hop_len=200, **kw)
    with pytest.raises(ValueError, match="'host' or 'device'"):
        infer_pipelined(2, lambda lo, hi: feats[lo:hi], toy_forward(), decode='gpu', **kw)
    with pytest.raises(ValueError, match='CUDA'):        # no host stand-in behind decode='device'
        infer_pipelined(2, lambda lo, hi: feats[lo:hi], toy_forward(), decode='device', **kw)


# ---------------------------------------------------------------------------------------------------- fixture g28
@pytest.mark.parametrize('name', ['exact', 'leftover', 'triple', 'file', 'y2020'])
def test_g28_rows_from_the_host_functions(name, emu):
    from salsa_amd.crnn.decode import chunk_starts, rows_to_list
    from salsa_amd.crnn.postprocess import combine_chunks, to_dcase_rows
    meta, a = load_golden('g28_test_chunks')
    case = meta['cases'][name]
    cl, ch, nc, nf = case['chunk_len'], case['chunk_hop'], case['n_classes'], meta['n_frames']
    assert len(chunk_starts(nf, cl, ch)) == case['n_chunks']
    sed, xyz = g28_inputs(case, meta['logit_mean'])
    fs, fx = combine_chunks(sed, cl, ch, n_frames=nf), combine_chunks(xyz, cl, ch, n_frames=nf)
    ref = a['rows:' + name].astype(np.int64)
    rows = to_dcase_rows(fs, fx, sed_threshold=meta['sed_threshold'], n_classes=nc, max_nframes_per_file=nf,
                         eval_version=case['eval_version'], as_array=True)
    assert ref.shape == (case['n_rows'], 5 if case['eval_version'] == '2021' else 4) and np.array_equal(rows, ref)
    # the kernel's arithmetic, serially on the host, through rows_to_list
    out = np.full((nf * nc, 4), -7, dtype=np.int16)
    n = emu.emu_decode(_fp(sed), _fp(xyz), case['n_chunks'], cl, ch, nf, nc, meta['sed_threshold'], 0, _sp(out))
    assert n == ref.shape[0] and (out[n:] == -7).all()
    got = rows_to_list(out[None], np.array([n]), eval_version=case['eval_version'], as_array=True)[0]
    assert got.dtype == np.int64 and got.shape == ref.shape and np.array_equal(got[:, :-2], ref[:, :-2])
    x, y, z = (fx[ref[:, 0], k * nc + ref[:, 1]] for k in range(3))
    azi, ele = angles64(x, y, z)
    assert_angles(got[:, -2], ref[:, -2], azi, name + ' azimuth')
    assert_angles(got[:, -1], ref[:, -1], ele, name + ' elevation')
    as_list = rows_to_list(out[None], np.array([n]), eval_version=case['eval_version'])[0]
    assert as_list == got.tolist() and isinstance(as_list[0][0], int)


# ---------------------------------------------------------------------------------------------------- split and frames
@pytest.mark.parametrize('T,cl,ch', [(960, 320, 200), (960, 320, 160), (960, 320, 320), (100, 30, 7), (960, 960, 962)])
def test_split_test_chunks_is_slicing_at_the_segment_starts(T, cl, ch):
    from salsa_amd.crnn.decode import split_test_chunks
    from salsa_amd.dataset import get_segment_idxes
    feat = torch.randn(3, 2, T, 5, generator=torch.Generator().manual_seed(T + cl))
    starts, _ = get_segment_idxes(T, cl, ch, 1, 0)
    assert ((T - cl) % ch != 0) == (starts[-1] != (len(starts) - 1) * ch)            # (with and without a leftover chunk)
    want = torch.stack([feat[b, :, s:s + cl] for b in range(3) for s in starts])  # file-major
    got = split_test_chunks(feat, cl, ch)
    assert got.shape == (3 * len(starts), 2, cl, 5) and got.is_contiguous() and torch.equal(got, want)


def test_test_chunk_frames():
    from salsa_amd.crnn.decode import chunk_starts, test_chunk_frames
    from salsa_amd.dataset import get_segment_idxes
    assert test_chunk_frames(4.0, 2.0) == ((320, 160), (40, 20))                    # the reference Database's defaults
    assert len(get_segment_idxes(4800, 320, 160, 1, 0)[0]) == len(chunk_starts(600, 40, 20)) == 29
    feat, lab = test_chunk_frames(60.0, 60.1)                                        # seld.yml: the whole clip at once
    assert feat == (4800, 4808) and lab == (600, 601)
    assert get_segment_idxes(4800, feat[0], feat[1], 1, 0)[0] == [0] and chunk_starts(600, *lab) == [0]
    assert test_chunk_frames(8.0, 0.5, fs=24000, hop_len=150) == ((1280, 80), (80, 5))


# ---------------------------------------------------------------------------------------------------- seld_decode.h on the host
@pytest.mark.parametrize('method', ['mean', 'gmean'])
@pytest.mark.parametrize('nf,cl,hop', [(120, 40, 25), (120, 40, 40), (120, 40, 15), (120, 120, 120), (100, 40, 25), (100, 33, 1),
                                       (100, 99, 98), (97, 40, 40), (600, 160, 60)])
def test_hostemu_combine_is_bit_equal_to_numpy(emu, method, nf, cl, hop):
    from salsa_amd.crnn.decode import chunk_starts
    from salsa_amd.crnn.postprocess import combine_chunks
    n = len(chunk_starts(nf, cl, hop))
    assert emu.emu_expected_chunks(nf, cl, hop) == n
    g = np.random.default_rng(nf * 1000 + cl + hop)
    chunks = g.random((n, cl, 5), dtype=np.float32) * np.exp(g.normal(size=(n, cl, 1)) * 4).astype(np.float32)   # over decades
    chunks[g.random(chunks.shape) < 0.05] = 0.0
    want = combine_chunks(chunks, cl, hop, n_frames=nf, combine_method=method)
    got = emu_combine(emu, chunks, cl, hop, nf, method)
    assert got.dtype == want.dtype and np.array_equal(got, want)


def test_hostemu_single_chunk_is_trimmed_and_uncovered_frames_average_with_zero(emu):
    g = np.random.default_rng(3)
    chunk = g.random((1, 130, 4), dtype=np.float32)
    for hop in (130, 7, 1000):                                                     # one chunk longer than the file: placed, trimmed
        assert emu.emu_expected_chunks(120, 130, hop) == 1
        assert np.array_equal(emu_combine(emu, chunk, 130, hop, 120, 'mean'), chunk[0, :120])
    # one step of the walk where no earlier chunk left a value (the file array starts as 0.0): numpy's float32 expressions
    new = np.concatenate([g.random(50, dtype=np.float32), np.float32([0.0, 1e-45, 3e-39, 3.4e38, np.inf])])
    old = np.zeros_like(new)
    with np.errstate(invalid='ignore'):
        mean, gmean = (old + new) / 2, np.sqrt(old * new)
    for i, v in enumerate(new):
        assert np.float32(emu.emu_combine_step(0.0, v, 1, 0, 5, 0)).tobytes() == mean[i].tobytes()
        got = np.float32(emu.emu_combine_step(0.0, v, 1, 0, 5, 1))
        assert got.tobytes() == gmean[i].tobytes() or (np.isnan(got) and np.isnan(gmean[i]))
        assert np.float32(emu.emu_combine_step(0.25, v, 0, 0, 5, 0)).tobytes() == v.tobytes()       # chunk 0 is copied
        assert np.float32(emu.emu_combine_step(0.25, v, 1, 5, 5, 1)).tobytes() == v.tobytes()       # behind the overlap: overwritten
    a, b = g.random(2000, dtype=np.float32), g.random(2000, dtype=np.float32)
    got = np.float32([[emu.emu_combine_step(x, y, 2, 1, 5, m) for x, y in zip(a, b)] for m in (0, 1)])
    assert np.array_equal(got[0], (a + b) / 2) and np.array_equal(got[1], np.sqrt(a * b))


def test_hostemu_angles_round_like_numpy(emu):
    g = torch.Generator().manual_seed(11)
    xyz = torch.tanh(torch.randn(20000, 3, generator=g)).numpy()
    azi = np.empty(len(xyz), dtype=np.int16)
    ele = np.empty_like(azi)
    emu.emu_angles(_fp(xyz), len(xyz), _sp(azi), _sp(ele))
    x, y, z = xyz.T
    a64, e64 = angles64(x, y, z)
    # float64 numpy: the same expression in the same precision
    w = np.rint(a64).astype(np.int64)
    w[w == 180] = -180
    assert_angles(azi, w, a64, 'azimuth against float64')
    assert_angles(ele, np.rint(e64).astype(np.int64), e64, 'elevation against float64')
    # the reference's float32 numpy expression (to_dcase_rows: models/interfaces.py:240-241)
    w = np.around(np.arctan2(y, x) * 180.0 / np.pi).astype(np.int64)
    w[w == 180] = -180
    assert_angles(azi, w, a64, 'azimuth against float32')
    assert_angles(ele, np.around(np.arctan2(z, np.sqrt(x ** 2 + y ** 2)) * 180.0 / np.pi).astype(np.int64), e64, 'elevation against float32')
    assert azi.min() == -180 and azi.max() == 179 and ele.min() < -80 and ele.max() > 80


def test_hostemu_angle_edges(emu):
    """the 180 -> -180 wrap, the poles, the zero vector, near-ties: (x, y, z) -> (azimuth, elevation)"""
    known = [((-1, 0, 0), (-180, 0)), ((-1, -0.0, 0), (-180, 0)), ((-1, 1e-8, 0), (-180, 0)), ((-1, -1e-8, 0), (-180, 0)),
             ((-1, 0.0087, 0), (-180, 0)), ((-1, -0.0087, 0), (-180, 0)),          # 179.5015 rounds to 180, which is written -180
             ((-1, 0.0088, 0), (179, 0)), ((-1, -0.0088, 0), (-179, 0)),           # 179.4958
             ((0, 0, 1), (0, 90)), ((0, 0, -1), (0, -90)), ((0, 0, 0), (0, 0)), ((1, 1, 0), (45, 0)), ((1, -1, 0), (-45, 0)),
             ((0, 1, 0), (90, 0)), ((0, -1, 0), (-90, 0)), ((1, 0, 1), (0, 45)), ((1e-30, 1e-30, 1e-30), (45, 35)),
             ((0.3, -0.4, 1e-20), (-53, 0))]
    t = np.tan(np.radians(np.float64([0.5, 1.5, 2.5, 44.5])))                      # near-ties: whichever side the float32 input falls
    cases = [k for k, _ in known] + [(1, v, 0) for v in t] + [(1, 0, v) for v in t]
    xyz = np.ascontiguousarray(cases, dtype=np.float32)
    azi = np.empty(len(xyz), dtype=np.int16)
    ele = np.empty_like(azi)
    emu.emu_angles(_fp(xyz), len(xyz), _sp(azi), _sp(ele))
    x, y, z = xyz.T
    a64, e64 = angles64(x, y, z)
    wa = np.rint(a64).astype(np.int64)
    wa[wa == 180] = -180
    assert np.array_equal(azi, wa) and np.array_equal(ele, np.rint(e64).astype(np.int64))
    assert [(int(a), int(e)) for a, e in zip(azi[:len(known)], ele[:len(known)])] == [w for _, w in known]
    assert not (azi == 180).any()


# ---------------------------------------------------------------------------------------------------- the export
def test_seld_decode_is_declared_listed_and_built_from_its_own_source():
    from salsa_amd import _lib
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'salsa_nn.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+salsa_nn_seld_decode\s*\(', hdr) and 'salsa_nn_seld_decode' in _lib.NN_EXPORTS
    assert os.path.join(ROOT, 'salsa_amd', 'csrc', 'seld_decode.hip') in _lib.build_command()
    src = open(os.path.join(ROOT, 'salsa_amd', 'csrc', 'seld_decode.hip')).read()
    assert '#include "seld_decode.h"' in src and '#include "build_guard.h"' in src


@pytest.fixture(scope='module')
def lib():
    from salsa_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_launcher_refuses_invalid_arguments_before_any_device_call(lib):
    """every call here returns -1 from the host-side checks: nothing is launched, no pointer is read (they point nowhere)"""
    assert lib.salsa_abi_version() == 2
    p = {k: C.c_void_p(0x1000 * (i + 1)) for i, k in enumerate(('sed', 'xyz', 'rows', 'counts'))}
    good = dict(n_files=2, n_chunks=5, chunk_len=40, chunk_hop=25, n_frames=120, nc=12, combine=0, **p)

    def call(**kw):
        a = dict(good, **kw)
        return lib.salsa_nn_seld_decode(a['sed'], a['xyz'], a['n_files'], a['n_chunks'], a['chunk_len'], a['chunk_hop'], a['n_frames'],
                                        a['nc'], 0.3, a['combine'], a['rows'], a['counts'], None, None, None)
    for k in p:
        assert call(**{k: None}) == -1, k                                          # a NULL required pointer
    assert call(rows=C.c_void_p(0x1004)) == -1                                     # rows are stored 8 bytes at a time
    assert call(n_frames=32768, n_chunks=1311) == -1                               # (1311 = the starts of 32768 frames: only the size is wrong)
    assert call(nc=0) == -1 and call(nc=-3) == -1
    assert call(chunk_hop=0) == -1 and call(chunk_hop=-25) == -1
    assert call(chunk_len=0, n_chunks=1) == -1 and call(chunk_len=-40) == -1
    for n in (1, 4, 6, 0, -1):
        assert call(n_chunks=n) == -1, n                                           # 5 starts: 0, 25, 50, 75 and the leftover 80
    assert call(chunk_hop=40, n_chunks=4) == -1 and call(chunk_hop=40, n_chunks=2) == -1      # (exactly 3 without overlap)
    assert call(chunk_hop=41, n_chunks=2) == -1 and call(chunk_hop=41, n_chunks=3) == -1      # hop > chunk_len with several chunks
    assert call(chunk_len=130, chunk_hop=10, n_chunks=2) == -1                     # chunk_len > n_frames with several chunks
    assert call(chunk_len=120, chunk_hop=120, n_chunks=2) == -1                    # a whole-file chunk is ONE chunk
    assert call(combine=2) == -1 and call(combine=-1) == -1
    assert call(n_files=0) == -1
