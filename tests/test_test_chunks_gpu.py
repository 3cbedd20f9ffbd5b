"""GPU tests of salsa_nn_seld_decode (test-time chunk combination + DCASE row decoding in one launch) and of the paths onto it:
the kernel against the host functions (postprocess.combine_chunks + to_dcase_rows) on built inputs, fixtures g28 and g25 through
decode_dcase_rows, run-to-run identity, and infer_pipelined with decode='device' against decode='host' on the same forward outputs.

What is compared how: the (frame, class) columns, the counts and the combined float arrays with array_equal, always.  Angles follow
the KNIFE-EDGE rule: the kernel computes them in float64, numpy's reference expression in float32 (largest deviation from float64
measured at 2.6e-5 degrees over 4e6 tanh(N(0, 1)) triples), so azimuth and elevation must be EQUAL wherever the float64 angle is more
than 1e-4 degrees from a half-integer and may differ by 1 inside that band (179 and -180 adjacent); at most 0.1 % of the active
pairs of a test's input may lie in the band (measured: 0.04 %), asserted before the allowance is used."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
BAND_DEG, BAND_CAP, SENTINEL, THR = 1e-4, 1e-3, -7, 0.3
EDGES = (0, 63, 64, 255, 256, -1)                        # flat pair indices: wave and tile boundaries, the last pair


def host_rows(sed, xyz, cl, hop, nf, nc, thr, method):
    """the yardstick: per file combine_chunks + to_dcase_rows (4 columns) -> (rows list, file_sed, file_xyz)"""
    from salsa_amd.crnn.postprocess import combine_chunks, to_dcase_rows
    rows, fs, fx = [], [], []
    with np.errstate(invalid='ignore'):
        for f in range(sed.shape[0]):
            fs.append(combine_chunks(sed[f], cl, hop, n_frames=nf, combine_method=method)[:nf])
            fx.append(combine_chunks(xyz[f], cl, hop, n_frames=nf, combine_method=method)[:nf])
            rows.append(to_dcase_rows(fs[-1], fx[-1], sed_threshold=thr, n_classes=nc, max_nframes_per_file=nf, eval_version='2020',
                                      as_array=True))
    return rows, np.stack(fs), np.stack(fx)


def exact_angles(rows, file_xyz, nc):
    """the float64 azimuth and elevation of the pairs named by per-file rows (frame, class, ..) in the combined directions"""
    f = np.concatenate([np.full(len(r), i) for i, r in enumerate(rows)])
    w = np.concatenate(rows).astype(np.int64)
    x, y, z = (file_xyz[f, w[:, 0], k * nc + w[:, 1]].astype(np.float64) for k in range(3))
    return np.arctan2(y, x) * 180.0 / np.pi, np.arctan2(z, np.sqrt(x ** 2 + y ** 2)) * 180.0 / np.pi


def in_band(a):
    return np.abs((a - np.floor(a)) - 0.5) <= BAND_DEG


def band_share(rows, file_xyz, nc):
    azi, ele = exact_angles(rows, file_xyz, nc)
    return float((in_band(azi) | in_band(ele)).mean()) if len(azi) else 0.0


def assert_rows(got, want, file_xyz, nc, what):
    """got / want: per file (n, 4) integer rows; file_xyz (files, frames, 3 nc) the combined directions: the module's rule"""
    assert [len(g) for g in got] == [len(w) for w in want], what
    g, w = np.concatenate(got).astype(np.int64), np.concatenate(want).astype(np.int64)
    assert np.array_equal(g[:, :2], w[:, :2]), what
    share = band_share(want, file_xyz, nc)
    assert share <= BAND_CAP, '%s: %.3f %% of %d active pairs lie in the rounding band' % (what, 100 * share, len(w))
    n_off = 0
    for col, exact in zip((2, 3), exact_angles(want, file_xyz, nc)):
        b = in_band(exact)
        diff = np.abs(g[:, col] - w[:, col])
        diff = np.minimum(diff, 360 - diff)
        assert not diff[~b].any() and diff.max(initial=0) <= 1, '%s column %d: %d differ outside the band' % (what, col, int((diff[~b] != 0).sum()))
        n_off += int((diff != 0).sum())
    print('%s: %d rows, %.3f %% in the band, %d angles off by one inside it' % (what, len(w), 100 * share, n_off))


def build(shape, cl, hop, method, pattern, seed):
    """(n_files, n_frames, nc) -> chunk activities and directions (numpy float32).  About 10 % of the chunk activities pass the
    threshold; for gmean the directions lie in the first octant (the root of a negative product is NaN and the root of a product
    of two negatives is positive, in the reference too: its geometric mean is for non-negative values; mean covers every octant).
    pattern shapes file 0 (file 1 for 'all'): see the test."""
    from salsa_amd.crnn.decode import chunk_starts
    n_files, nf, nc = shape
    starts = chunk_starts(nf, cl, hop)
    g = torch.Generator().manual_seed(seed)
    sed = torch.rand(n_files, len(starts), cl, nc, generator=g) * (THR / 0.9)
    xyz = torch.tanh(torch.randn(n_files, len(starts), cl, 3 * nc, generator=g))
    if method == 'gmean':
        xyz = xyz.abs()

    def place(f, file_sed):                              # chunks that all say what the file array says: they combine to it
        for i, s in enumerate(starts):
            sed[f, i] = file_sed[s:s + cl]
    if pattern == 'none':
        place(0, torch.zeros(nf, nc))
    elif pattern == 'all':
        place(1, torch.full((nf, nc), 0.75))
    elif pattern == 'edges':
        flat = torch.zeros(nf * nc)
        flat[list(EDGES)] = 0.75
        place(0, flat.reshape(nf, nc))
    elif pattern == 'nan':
        sed[0][torch.rand(sed[0].shape, generator=g) < 0.05] = float('nan')
        sed[0, 0, 0, 0] = float('nan')
        sed[0, -1, -1, -1] = float('nan')
    else:
        assert pattern == 'random'
    return sed.numpy(), xyz.numpy()


def run_kernel(sed, xyz, cl, hop, nf, thr, method, file_outputs=True):
    """one salsa_nn_seld_decode call on a stream of its own, every output pre-filled -> host arrays (rows, counts, file_sed, file_xyz)"""
    from salsa_amd import _lib
    n_files, n_chunks, _, nc = sed.shape
    stream = torch.cuda.Stream(DEV)
    assert stream != torch.cuda.default_stream(DEV)
    with torch.cuda.stream(stream):
        s, x = torch.from_numpy(sed).to(DEV), torch.from_numpy(xyz).to(DEV)
        rows = torch.full((n_files, nf * nc, 4), SENTINEL, dtype=torch.int16, device=DEV)
        counts = torch.full((n_files,), -1, dtype=torch.int32, device=DEV)
        fs = torch.full((n_files, nf, nc), float('nan'), device=DEV) if file_outputs else None
        fx = torch.full((n_files, nf, 3 * nc), float('nan'), device=DEV) if file_outputs else None
        ptr = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None          # noqa: E731
        rc = _lib.load().salsa_nn_seld_decode(ptr(s), ptr(x), n_files, n_chunks, cl, hop, nf, nc, thr, int(method == 'gmean'), ptr(rows),
                                              ptr(counts), ptr(fs), ptr(fx), C.c_void_p(stream.cuda_stream))
        assert rc == 0
    stream.synchronize()
    return rows.cpu().numpy(), counts.cpu().numpy(), None if fs is None else fs.cpu().numpy(), None if fx is None else fx.cpu().numpy()


CHUNKINGS = {120: ((40, 25), (40, 40), (40, 15), (120, 120)), 100: ((40, 25), (40, 40), (40, 15), (100, 100))}


@pytest.mark.parametrize('pattern', ['random', 'none', 'all', 'edges', 'nan'])
@pytest.mark.parametrize('method', ['mean', 'gmean'])
@pytest.mark.parametrize('chunking', range(4))
@pytest.mark.parametrize('shape', [(3, 120, 12), (2, 100, 14)])
def test_kernel_against_the_host_functions(shape, chunking, method, pattern):
    """leftover chunk / no overlap / triple coverage / one chunk, at 1440 pairs (5.6 tiles) and 1400 pairs; a file with nothing
    active, one with every pair active (count = capacity), active pairs exactly at the wave and tile boundaries, NaN activities"""
    n_files, nf, nc = shape
    cl, hop = CHUNKINGS[nf][chunking]
    # these inputs have a few hundred active pairs, so the 0.1 % cap admits none of them in the band: the draw is repeated with the
    # next seed until the INPUT meets the cap (a property of the input alone, judged in float64 on the host before the kernel runs)
    for seed in range(nf + 7 * chunking + (100 if method == 'gmean' else 0), 10 ** 6, 1000):
        sed, xyz = build(shape, cl, hop, method, pattern, seed)
        want, fs, fx = host_rows(sed, xyz, cl, hop, nf, nc, THR, method)
        if band_share(want, fx, nc) <= BAND_CAP:
            break
    assert np.isfinite(fx).all()
    rows, counts, gfs, gfx = run_kernel(sed, xyz, cl, hop, nf, THR, method)
    what = '%s chunks (%d, %d) %s %s' % (shape, cl, hop, method, pattern)
    assert np.array_equal(counts, [len(w) for w in want]), what
    assert np.array_equal(gfs, fs, equal_nan=True) and np.array_equal(gfx, fx), what
    for f in range(n_files):
        assert (rows[f, counts[f]:] == SENTINEL).all(), (what, f)                # nothing is written behind the count
    assert_rows([rows[f, :counts[f]] for f in range(n_files)], want, fx, nc, what)
    frac = counts.sum() / (n_files * nf * nc)
    if pattern == 'random':
        assert 0.02 < frac < 0.15
    elif pattern == 'none':
        assert counts[0] == 0 and counts[1:].min() > 0
    elif pattern == 'all':
        assert counts[1] == nf * nc and counts[0] < nf * nc
    elif pattern == 'edges':
        flat = rows[0, :counts[0], 0].astype(np.int64) * nc + rows[0, :counts[0], 1]
        assert list(flat) == [e % (nf * nc) for e in EDGES]
    else:
        assert np.isnan(fs[0]).sum() > 20 and not (fs[0][np.isnan(fs[0])] >= THR).any() and counts[0] > 0
    rows2, counts2, none_s, none_x = run_kernel(sed, xyz, cl, hop, nf, THR, method, file_outputs=False)
    assert none_s is None and none_x is None and np.array_equal(rows2, rows) and np.array_equal(counts2, counts)   # (NULL file outputs)


def test_two_runs_are_bit_identical():
    sed, xyz = build((3, 120, 12), 40, 15, 'mean', 'random', seed=1)
    a, b = run_kernel(sed, xyz, 40, 15, 120, THR, 'mean'), run_kernel(sed, xyz, 40, 15, 120, THR, 'mean')
    assert a[1].sum() > 100
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()


def test_wrapper_refuses_what_the_kernel_refuses_and_cpu_tensors():
    from salsa_amd.crnn.decode import decode_dcase_rows
    sed, xyz = torch.rand(2, 5, 40, 12, device=DEV), torch.rand(2, 5, 40, 36, device=DEV)
    rows, counts = decode_dcase_rows(sed, xyz, 40, 25, n_frames=120)
    assert rows.shape == (2, 1440, 4) and rows.dtype == torch.int16 and counts.dtype == torch.int32 and rows.is_cuda
    with pytest.raises(ValueError, match='expected 4 chunks'):
        decode_dcase_rows(sed, xyz, 40, 30, n_frames=120)
    with pytest.raises(ValueError, match='CUDA'):
        decode_dcase_rows(sed.cpu(), xyz.cpu(), 40, 25, n_frames=120)
    with pytest.raises(ValueError, match='unknown'):
        decode_dcase_rows(sed, xyz, 40, 25, n_frames=120, combine_method='median')


@pytest.mark.parametrize('name', ['exact', 'leftover', 'triple', 'file', 'y2020'])
def test_g28_through_decode_dcase_rows(name):
    from salsa_amd.crnn.decode import decode_dcase_rows, rows_to_list
    from salsa_amd.crnn.postprocess import combine_chunks
    meta, a = load_golden('g28_test_chunks')
    case = meta['cases'][name]
    g = torch.Generator().manual_seed(case['seed'])
    logit = torch.randn(case['n_chunks'], case['chunk_len'], case['n_classes'], generator=g) + meta['logit_mean']
    xyz = torch.tanh(torch.randn(case['n_chunks'], case['chunk_len'], 3 * case['n_classes'], generator=g))
    sed = torch.sigmoid(logit)                                                     # on the CPU, as the reference does
    rows, counts, fs, fx = decode_dcase_rows(sed[None].to(DEV), xyz[None].to(DEV), case['chunk_len'], case['chunk_hop'],
                                             n_frames=meta['n_frames'], sed_threshold=meta['sed_threshold'], return_file_outputs=True)
    ref = a['rows:' + name].astype(np.int64)
    got = rows_to_list(rows.cpu(), counts.cpu(), eval_version=case['eval_version'], as_array=True)[0]
    assert got.shape == ref.shape
    if case['eval_version'] == '2021':
        assert not got[:, 2].any() and not ref[:, 2].any()
        got, ref = got[:, [0, 1, 3, 4]], ref[:, [0, 1, 3, 4]]
    wfs, wfx = (combine_chunks(t.numpy(), case['chunk_len'], case['chunk_hop'], n_frames=meta['n_frames']) for t in (sed, xyz))
    assert np.array_equal(fs.cpu().numpy()[0], wfs) and np.array_equal(fx.cpu().numpy()[0], wfx)
    assert_rows([got], [ref], wfx[None], case['n_classes'], 'g28 ' + name)


def test_g25_chunked_accdoa_rows():
    """accdoa: the SED decision per chunk (salsa_nn_accdoa_sed), then the chunks are combined -- the order the fixture pins"""
    from salsa_amd.crnn.decode import decode_dcase_rows, rows_to_list
    from salsa_amd.crnn.nn_ops import accdoa_sed
    from salsa_amd.crnn.postprocess import combine_chunks
    meta, a = load_golden('g25_accdoa')

    def accdoa_output(shape, g):                                                   # (tools/make_golden_accdoa.py draws them so)
        n, T, c3 = shape
        v = torch.randn(n, T, 3, c3 // 3, generator=g)
        v = v / v.norm(dim=2, keepdim=True) * 0.6 * torch.rand(n, T, 1, c3 // 3, generator=g)
        return v.reshape(n, T, c3).numpy().astype(np.float32)
    g = torch.Generator().manual_seed(meta['rows_seed'])
    accdoa_output((1, 600, 36), g)                                                 # (the whole-file case is drawn first)
    doa = accdoa_output((meta['n_chunks'], meta['chunk_len'], 36), g)
    xyz = torch.from_numpy(doa).to(DEV)
    rows, counts = decode_dcase_rows(accdoa_sed(xyz, 12)[None], xyz[None], meta['chunk_len'], meta['chunk_hop'])
    got = rows_to_list(rows.cpu(), counts.cpu(), as_array=True)[0]
    ref = a['rows:chunks'].astype(np.int64)
    assert got.shape == ref.shape and not got[:, 2].any()
    fx = combine_chunks(doa, meta['chunk_len'], meta['chunk_hop'])
    assert_rows([got[:, [0, 1, 3, 4]]], [ref[:, [0, 1, 3, 4]]], fx[None], 12, 'g25 rows:chunks')


@pytest.fixture(scope='module')
def trainer():
    from salsa_amd.crnn.train import Trainer
    torch.manual_seed(0)
    return Trainer(DEV, total_steps=10 ** 6)


@pytest.mark.parametrize('chunked', [True, False])
def test_infer_pipelined_device_rows_equal_host_rows(trainer, chunked):
    """a real Trainer's forward, recorded once; both decode paths then get the SAME tensors.  5 clips at sub_batch 2: the last
    sub-batch is partial.  chunked: 320 / 200 feature frames = 40 / 25 label frames of 120 (a leftover chunk); else whole clips."""
    from salsa_amd.crnn.infer import infer_pipelined
    from salsa_amd.crnn.postprocess import combine_chunks
    tr = trainer
    kw = dict(chunk_len=320, chunk_hop_len=200) if chunked else {}
    # a few hundred active pairs: the 0.1 % cap admits none in the rounding band, so the clips are redrawn with the next seed until
    # the forward's recorded outputs meet it (a property of the decoders' INPUT, judged in float64 on the host)
    for seed in range(9, 17):
        feats = torch.randn(5, 7, 960, 200, generator=torch.Generator().manual_seed(seed)).to(DEV)
        with torch.no_grad():
            thr = float(torch.quantile(tr.infer(feats[:1, :, :320] if chunked else feats[:1])[0].flatten(), 0.9))
        tape = []

        def record(x):
            tape.append(tr.infer(x))
            return tape[-1]
        host = infer_pipelined(5, lambda lo, hi: feats[lo:hi], record, sub_batch=2, depth=2, sed_threshold=thr, n_label_frames=120,
                               decode='host', eval_version='2020', as_array=True, **kw)
        xyz = torch.cat([t[1] for t in tape]).cpu().numpy()
        fx = np.stack([combine_chunks(c, 40, 25, n_frames=120) for c in xyz.reshape(5, 5, 40, 36)]) if chunked else xyz
        if band_share(host, fx, 12) <= BAND_CAP:
            break
    assert len(tape) == (5 if chunked else 3) and tape[0][0].shape[1] == (40 if chunked else 120)
    replay = iter(tape)
    dev = infer_pipelined(5, lambda lo, hi: feats[lo:hi], lambda x: next(replay), sub_batch=2, depth=2, sed_threshold=thr,
                          n_label_frames=120, decode='device', eval_version='2020', as_array=True, **kw)
    assert next(replay, None) is None
    assert sum(len(r) for r in host) > 200
    assert_rows(dev, host, fx, 12, 'infer_pipelined %s (clip seed %d)' % ('chunks 320 / 200' if chunked else 'whole clips', seed))
    lists = infer_pipelined(5, lambda lo, hi: feats[lo:hi], lambda x, it=iter(tape): next(it), sub_batch=2, sed_threshold=thr,
                            n_label_frames=120, decode='device', **kw)
    assert [len(r) for r in lists] == [len(r) for r in dev] and all(len(row) == 5 and row[2] == 0 for r in lists for row in r)
