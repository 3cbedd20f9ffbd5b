"""GPU tests of per-class SED thresholds and the one-launch threshold sweep: salsa_nn_seld_decode_thr /
salsa_nn_seld_decode_multi_thr against the host decoders, salsa_nn_seld_sweep (crnn/calibrate.py::sweep_outputs) against the host twin
sweep_host on the planted case of tests/sweep_reference.py (3 files x 25 frames at label rate 10, 3 classes, 6 candidates), at the
limits (32 classes x 64 candidates) and on the seeded random case (2 files x 600 x 12, K = 17), its output discipline, the launcher's
refusals, the selection, and infer_pipelined(sweep=) / validate(calibrate=) end to end.

Bounds.  Rows and counts of the decoders: bit-equal to the host's.  The sweep after host resolution: every integer equal to
sweep_host's, total_DE within DE_TP x margin (crnn.score.DEFAULT_MARGIN: the device's distances are not numpy's bit for bit, at most
1.2e-6 degrees apart each, and the device adds per segment and then the segments).  The status array is EQUAL to what numpy's own
distances say (sweep_reference.expected_status), so the planted doubt and refused entries are counted exactly."""
import ctypes as C

import numpy as np
import pytest
import torch

import sweep_reference as ref

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def margin():
    from salsa_amd.crnn.score import DEFAULT_MARGIN
    return DEFAULT_MARGIN


def on_device(case):
    from salsa_amd.crnn.score import gt_rows_to_device
    gt_rows, gt_counts = gt_rows_to_device(case['gt'], DEV)
    return torch.from_numpy(case['act']).to(DEV), torch.from_numpy(case['xyz']).to(DEV), gt_rows, gt_counts


def host_sweep(case, n_frames, n_classes, rate=ref.RATE):
    from salsa_amd.crnn.calibrate import sweep_host
    return sweep_host(case['act'], case['xyz'], case['gt'], case['thresholds'], n_frames=n_frames, n_classes=n_classes, label_rate=rate,
                      output_format=case['fmt'], unify_deg=case['unify_deg'])


def device_sweep(case, n_frames, n_classes, rate=ref.RATE):
    from salsa_amd.crnn.calibrate import sweep_outputs
    act, xyz, gt_rows, gt_counts = on_device(case)
    return sweep_outputs(act, xyz, gt_rows, gt_counts, case['thresholds'], n_frames=n_frames, n_classes=n_classes, label_rate=rate,
                         output_format=case['fmt'], unify_deg=case['unify_deg'])


def assert_equal_sweeps(dev, host):
    assert (dev.counters == host.counters).all()
    print('max |total_DE device - host| = %g over DE_TP up to %d' % (np.abs(dev.total_DE - host.total_DE).max(), host.counters[..., 5].max()))
    assert (np.abs(dev.total_DE - host.total_DE) <= host.counters[..., 5] * margin()).all()


@pytest.fixture(scope='module', params=['reg_xyz', 'multi_accdoa'])
def planted(request):
    case = ref.planted_case(request.param)
    return case, host_sweep(case, ref.N_FRAMES, ref.C)


# ------------------------------------------------------------------------------------------------------- the decoders
def test_decoders_with_a_threshold_vector_equal_the_host_and_the_scalar_entries(planted):
    from salsa_amd.crnn.decode import decode_dcase_rows, decode_multi_rows, rows_to_list
    case, _ = planted
    act, xyz, _, _ = on_device(case)
    multi = case['fmt'] == 'multi_accdoa'

    def decode(thr):
        if multi:
            rows, counts = decode_multi_rows(act, xyz, n_frames=ref.N_FRAMES, sed_threshold=thr, unify_deg=15.0, n_classes=ref.C)
        else:
            rows, counts = decode_dcase_rows(act, xyz, ref.N_FRAMES, ref.N_FRAMES, n_frames=ref.N_FRAMES, sed_threshold=thr)
        return rows.cpu(), counts.cpu()
    for vec in (np.array([0.2, 0.5, 0.3]), case['thresholds'][2], [0.3, float('nan'), 0.05], case['thresholds'][0]):
        rows, counts = decode(vec)
        got = rows_to_list(rows, counts, eval_version='2020')
        want = [ref.host_rows(case['act'][f], case['xyz'][f], vec, ref.N_FRAMES, ref.C, case['fmt'], 15.0) for f in range(ref.N_FILES)]
        assert got == want and sum(map(len, got)) > 0
    for same in (0.3, 0.5):                                                                      # equal entries: the scalar entry's bits
        (r_vec, c_vec), (r_scalar, c_scalar) = decode([same] * ref.C), decode(same)
        assert torch.equal(c_vec, c_scalar) and all(torch.equal(r_vec[f, :c_vec[f]], r_scalar[f, :c_scalar[f]]) for f in range(ref.N_FILES))
    if not multi:                                                                                # the combined file outputs too, to the bit
        for same in (0.3, 0.5):
            vec_out = decode_dcase_rows(act, xyz, ref.N_FRAMES, ref.N_FRAMES, n_frames=ref.N_FRAMES, sed_threshold=[same] * ref.C, return_file_outputs=True)
            scalar_out = decode_dcase_rows(act, xyz, ref.N_FRAMES, ref.N_FRAMES, n_frames=ref.N_FRAMES, sed_threshold=same, return_file_outputs=True)
            for v, s_ in zip(vec_out[2:], scalar_out[2:]):
                assert v.cpu().numpy().tobytes() == s_.cpu().numpy().tobytes()                   # (bytes: the planted NaNs compare too)
            assert vec_out[2].cpu().numpy().tobytes() == case['act'].tobytes()                   # one chunk per file: placed, no arithmetic
    uploaded = torch.tensor([0.2, 0.5, 0.3], dtype=torch.float32, device=DEV)                    # a vector uploaded once by the caller
    (r_t, c_t), (r_v, c_v) = decode(uploaded), decode([0.2, 0.5, 0.3])
    assert torch.equal(c_t, c_v) and all(torch.equal(r_t[f, :c_t[f]], r_v[f, :c_v[f]]) for f in range(ref.N_FILES))
    for bad in ([0.3, 0.3], uploaded.cpu(), uploaded.double(), uploaded[:2]):
        with pytest.raises(ValueError, match='sed_threshold'):
            decode(bad)


# ------------------------------------------------------------------------------------------------------- the sweep
def test_sweep_equals_sweep_host_on_the_planted_case(planted):
    from salsa_amd.crnn.calibrate import PendingSweep
    case, host = planted
    act, xyz, gt_rows, gt_counts = on_device(case)
    pending = PendingSweep(act, xyz, gt_rows, gt_counts, case['thresholds'], ref.N_FRAMES, ref.C, ref.DOA_THRESHOLD, ref.RATE, margin(),
                           case['fmt'], case['unify_deg'])
    dev = pending.result()
    status = pending.host['status'].numpy()
    want = ref.expected_status(case['act'], case['xyz'], case['gt'], case['thresholds'], ref.N_FRAMES, ref.C, case['fmt'], case['unify_deg'], margin())
    assert (status == want).all()
    assert (np.argwhere(status == 1) == [[1, 0, k, 2] for k in (1, 2, 3, 4)]).all() and (status == 1).sum() == 4      # the 20-degree slot
    assert (np.argwhere(status == 2) == [[1, 1, k, 0] for k in range(6)]).all() and (status == 2).sum() == 6          # the 5-DOA cell
    assert (dev.n_entries, dev.n_doubt, dev.n_refused) == (3 * 3 * 6 * 3, 4, 6)
    counters, class_de, _ = (t.cpu().numpy() for t in pending.records)
    flat = status.reshape(-1, 6, 3)
    assert not counters[flat != 0].any() and not class_de[flat != 0].any()                       # such entries carry zeros
    assert_equal_sweeps(dev, host)


def test_sweep_at_the_limits():
    """32 classes x 64 candidates, every (k, c) its own threshold; and Multi-ACCDOA at label rate 32, where the classes are walked
    in groups of four"""
    for fmt, rate, K in (('reg_xyz', 10, 64), ('multi_accdoa', 32, 8)):
        n_frames = 2 * rate + 3
        act, xyz, gt = ref.random_case(5, 1, n_frames, 32, fmt, gt_density=0.3)
        thresholds = np.linspace(0.05, 1.0, K * 32, dtype=np.float32).reshape(32, K).T.copy()
        case = dict(act=act, xyz=xyz, gt=gt, thresholds=thresholds, fmt=fmt, unify_deg=15.0)
        dev = device_sweep(case, n_frames, 32, rate)
        assert dev.n_doubt + dev.n_refused <= 0.02 * dev.n_entries
        assert_equal_sweeps(dev, host_sweep(case, n_frames, 32, rate))


@pytest.fixture(scope='module')
def random_case():
    act, xyz, gt = ref.random_case(ref.RANDOM_SEED, 2, 600, 12, 'reg_xyz')
    thresholds = np.repeat(np.linspace(0.1, 0.9, 17, dtype=np.float32)[:, None], 12, axis=1)
    case = dict(act=act, xyz=xyz, gt=gt, thresholds=thresholds, fmt='reg_xyz', unify_deg=15.0)
    return case, host_sweep(case, 600, 12)


def test_sweep_on_the_seeded_random_case_and_the_composed_path(random_case, monkeypatch):
    case, host = random_case
    dev = device_sweep(case, 600, 12)
    assert dev.n_entries == 2 * 60 * 17 * 12 and dev.n_doubt + dev.n_refused <= 0.02 * dev.n_entries    # (the seed was checked on the CPU)
    assert_equal_sweeps(dev, host)
    monkeypatch.setenv('SALSA_HIP_SWEEP', '0')                                                   # K x (decode + score 2022)
    composed = device_sweep(case, 600, 12)
    assert_equal_sweeps(composed, host)
    assert (composed.counters == dev.counters).all()


def test_selection_on_the_device_equals_the_host(random_case):
    case, host = random_case
    dev = device_sweep(case, 600, 12)
    J = host.classwise()[..., 3]
    (h_thr, h_idx), (d_thr, d_idx) = host.best(), dev.best()
    band = 0
    for c in range(12):
        order = np.argsort(J[:, c], kind='stable')
        if J[order[1], c] - J[order[0], c] > 2 * margin() / 540:                                 # J moves by at most margin / 540 per side
            assert d_idx[c] == h_idx[c] and d_thr[c] == h_thr[c]
        else:
            band += 1
            assert d_idx[c] in (order[0], order[1])
    assert band <= 1 and len(set(h_idx.tolist())) > 1                                            # the classes do differ in their best candidate


# ------------------------------------------------------------------------------------------------------- output discipline
def raw_sweep(case, act, xyz, gt_rows, gt_counts, n_frames, n_classes, guard=64):
    """one salsa_nn_seld_sweep call into sentinel-filled buffers with guard bands -> the five outputs as numpy, guards checked"""
    from salsa_amd import _lib
    from salsa_amd.crnn.postprocess import cos_unify_of
    n, K = act.shape[0], case['thresholds'].shape[0]
    n_seg = -(-n_frames // ref.RATE)
    thr = torch.from_numpy(np.ascontiguousarray(case['thresholds'], np.float32)).to(DEV)
    shapes = dict(counters=((n * n_seg * K * n_classes * 5,), torch.int32), de=((n * n_seg * K * n_classes,), torch.float64),
                  status=((n * n_seg * K * n_classes,), torch.int32), sums=((n * K * n_classes * 5,), torch.int64), sum_de=((n * K * n_classes,), torch.float64))
    buf = {k: (torch.full((s[0] + 2 * guard,), float('nan'), dtype=dt, device=DEV) if dt == torch.float64
               else torch.full((s[0] + 2 * guard,), -77, dtype=dt, device=DEV)) for k, (s, dt) in shapes.items()}
    ptr = lambda t: C.c_void_p(t.data_ptr())
    inner = {k: buf[k][guard:-guard] for k in buf}
    multi = case['fmt'] == 'multi_accdoa'
    rc = _lib.load().salsa_nn_seld_sweep(ptr(act), ptr(xyz), n, act.shape[1], n_frames, n_classes, int(multi), cos_unify_of(15.0) if multi else 1.0,
                                         ptr(thr), K, ptr(gt_rows), ptr(gt_counts), gt_rows.shape[1], ref.RATE, 20.0, margin(),
                                         ptr(inner['counters']), ptr(inner['de']), ptr(inner['status']), ptr(inner['sums']), ptr(inner['sum_de']),
                                         C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    out = {}
    for k, t in buf.items():
        h = t.cpu().numpy()
        edge = np.concatenate([h[:guard], h[-guard:]])
        assert np.isnan(edge).all() if h.dtype == np.float64 else (edge == -77).all(), k         # nothing outside the outputs is touched
        out[k] = h[guard:-guard]
        assert not np.isnan(out[k]).any() if h.dtype == np.float64 else (out[k] >= 0).all(), k   # every element is overwritten
    return out


def test_every_output_is_written_twice_the_same_and_a_file_does_not_depend_on_its_batch(planted):
    case, _ = planted
    act, xyz, gt_rows, gt_counts = on_device(case)
    a = raw_sweep(case, act, xyz, gt_rows, gt_counts, ref.N_FRAMES, ref.C)
    b = raw_sweep(case, act, xyz, gt_rows, gt_counts, ref.N_FRAMES, ref.C)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)                                      # two launches: bit-identical
    alone = raw_sweep(case, act[1:2].contiguous(), xyz[1:2].contiguous(), gt_rows[1:2].contiguous(), gt_counts[1:2].contiguous(), ref.N_FRAMES, ref.C)
    for k in a:
        per_file = a[k].reshape(ref.N_FILES, -1)
        assert per_file[1].tobytes() == alone[k].tobytes(), k
    # a gt count its slab cannot hold: every entry of that file refused, with zeros, and nothing of it is read
    bad = gt_counts.clone()
    bad[2] = gt_rows.shape[1] + 1
    c = raw_sweep(case, act, xyz, gt_rows, bad, ref.N_FRAMES, ref.C)
    assert (c['status'].reshape(3, -1)[2] == 2).all() and not c['counters'].reshape(3, -1)[2].any() and not c['sums'].reshape(3, -1)[2].any()
    assert c['status'].reshape(3, -1)[:2].tobytes() == a['status'].reshape(3, -1)[:2].tobytes()
    from salsa_amd.crnn.calibrate import sweep_outputs
    with pytest.raises(ValueError, match='count'):
        sweep_outputs(act, xyz, gt_rows, bad, case['thresholds'], n_frames=ref.N_FRAMES, n_classes=ref.C, output_format=case['fmt'])


def test_launcher_refuses_bad_arguments_without_a_launch():
    from salsa_amd import _lib
    lib = _lib.load()
    names = ('act', 'xyz', 'thresholds', 'gt_rows', 'gt_counts', 'class_counters', 'class_de', 'status', 'file_counters', 'file_de')
    p = {k: C.c_void_p(0x1000 * (i + 1)) for i, k in enumerate(names)}                           # (they point nowhere: a launch would fault)
    good = dict(n_files=4, n_in=600, n_frames=600, n_classes=12, multi=1, cos=0.96, K=17, cap=900, rate=10, thr=20.0, margin=1e-4, **p)

    def call(**kw):
        a = dict(good, **kw)
        return lib.salsa_nn_seld_sweep(a['act'], a['xyz'], a['n_files'], a['n_in'], a['n_frames'], a['n_classes'], a['multi'], a['cos'], a['thresholds'],
                                       a['K'], a['gt_rows'], a['gt_counts'], a['cap'], a['rate'], a['thr'], a['margin'], a['class_counters'],
                                       a['class_de'], a['status'], a['file_counters'], a['file_de'], None)
    for k in names:
        assert call(**{k: None}) == _lib.E_INVAL and 'salsa_nn_seld_sweep' in _lib.last_error(), k
    assert call(gt_rows=C.c_void_p(0x1004)) == _lib.E_INVAL and 'misaligned' in _lib.last_error()
    for k, bad in (('n_classes', (0, 33)), ('rate', (0, 33)), ('K', (0, 65)), ('n_files', (0, 65536)), ('n_frames', (0, 32768)), ('n_in', (599,)),
                   ('cap', (0,)), ('multi', (2,)), ('cos', (float('nan'), 1.5)), ('margin', (-1e-9, float('nan'))), ('thr', (float('nan'),))):
        for v in bad:
            assert call(**{k: v}) == _lib.E_INVAL and 'salsa_nn_seld_sweep' in _lib.last_error(), (k, v)
    torch.cuda.synchronize()                                                                      # nothing was launched: nothing to fault
    from salsa_amd.crnn.calibrate import sweep_outputs
    case = ref.planted_case('reg_xyz')
    act, xyz, gt_rows, gt_counts = on_device(case)
    for bad in (np.zeros(65, np.float32), np.zeros((6, 4), np.float32)):
        with pytest.raises(ValueError, match='thresholds'):
            sweep_outputs(act, xyz, gt_rows, gt_counts, bad, n_frames=ref.N_FRAMES, n_classes=ref.C)
    with pytest.raises(ValueError, match='CUDA'):
        sweep_outputs(act.cpu(), xyz.cpu(), gt_rows, gt_counts, ref.GRID, n_frames=ref.N_FRAMES, n_classes=ref.C)


# ------------------------------------------------------------------------------------------------------- end to end
FRAMES, F, CHUNK, HOP = 256, 200, 128, 64
CANDIDATES = np.array([0.3, 0.45, 0.5, 0.55], np.float32)
FIGURES = ('valER', 'valF1', 'valLE', 'valLR', 'valSeld')


def test_infer_pipelined_sweep_with_chunks_tta_and_aligned_tracks():
    """a tiny Multi-ACCDOA trainer through overlapping chunks with tta= and track_merge='align': the sweep of decode='device' equals
    sweep_host on the combined outputs it kept, and the rows are those of the call without sweep="""
    from salsa_amd.crnn.calibrate import ThresholdSweep, sweep_host
    from salsa_amd.crnn.infer import infer_pipelined
    from salsa_amd.crnn.score import gt_rows_to_device
    from salsa_amd.crnn.train import Trainer
    torch.manual_seed(3)
    tr = Trainer(DEV, total_steps=10 ** 6, output_format='multi_accdoa', n_classes=2)
    tr.track_merge = 'align'
    feats = torch.randn(3, 7, 160, F, generator=torch.Generator().manual_seed(5)).to(DEV)
    rng = np.random.RandomState(2)
    gt = [[(int(f), int(rng.randint(2)), int(rng.randint(-180, 180)), int(rng.randint(-40, 40))) for f in range(0, 20, 2)] for _ in range(3)]
    gt_rows, gt_counts = gt_rows_to_device(gt, DEV)
    first = tr.infer(feats[:1, :, :64])[0].float().cpu().numpy()                                 # the scale of a fresh model's track activities
    thresholds = np.quantile(first, [0.2, 0.4, 0.6, 0.8]).astype(np.float32)
    vec = [float(thresholds[1]), float(thresholds[2])]
    kw = dict(sub_batch=2, sed_threshold=vec, n_label_frames=20, output_format='multi_accdoa', n_classes=2, eval_version='2020',
              chunk_len=64, chunk_hop_len=40, tta=('foa', 'salsa'), track_merge='align', decode='device')
    acc = ThresholdSweep(thresholds, 2, 20, 10)
    rows = infer_pipelined(3, lambda lo, hi: feats[lo:hi], tr.infer, sweep=(gt_rows, gt_counts, acc), **kw)
    assert rows == infer_pipelined(3, lambda lo, hi: feats[lo:hi], tr.infer, **kw) and sum(map(len, rows)) > 0
    assert acc.counters.shape == (3, 4, 2, 8) and [tuple(a.shape) for a, _ in acc.outputs] == [(2, 20, 6), (1, 20, 6)] and acc.outputs[0][0].is_cuda
    act = np.concatenate([a.cpu().numpy() for a, _ in acc.outputs])
    xyz = np.concatenate([x.cpu().numpy() for _, x in acc.outputs])
    host = sweep_host(act, xyz, gt, thresholds, n_frames=20, n_classes=2, output_format='multi_accdoa')
    assert_equal_sweeps(acc, host)
    from salsa_amd.crnn.postprocess import multi_accdoa_rows
    assert rows == [multi_accdoa_rows(act[f], xyz[f], sed_threshold=vec, n_classes=2, max_nframes_per_file=20, eval_version='2020') for f in range(3)]


def bank_from_files(tmp, n_clips, seed, nc=12):
    from salsa_amd import io as sio
    from salsa_amd.dataset import GpuFeatureBank
    g = torch.Generator().manual_seed(seed)
    files = [sio.save_arrays(str(tmp / ('s%d_clip%d.h5' % (seed, i))), feature=torch.randn(7, FRAMES, F, generator=g).numpy()) for i in range(n_clips)]
    sed = (torch.rand(n_clips, FRAMES // 8, nc, generator=g) < 0.2).float()
    v = torch.randn(n_clips, FRAMES // 8, 3, nc, generator=g)
    doa = ((v / v.norm(dim=2, keepdim=True)) * sed[:, :, None, :]).reshape(n_clips, FRAMES // 8, 3 * nc)
    bank = GpuFeatureBank(None, chunk_len_s=CHUNK / 80, chunk_hop_len_s=HOP / 80, n_classes=nc, device='cuda')
    bank.set_scaler(np.zeros((4, 1, F), np.float32), np.ones((4, 1, F), np.float32))
    bank.add_feature_files(files, sed=sed.numpy(), doa=doa.numpy())
    return bank.finalize()


def test_validate_calibrate_on_the_gpu_equals_validate_at_the_chosen_vector(tmp_path):
    """reg_xyz through overlapping chunks: one forward pass, then the figures of validate(sed_threshold=chosen) -- the scorer's
    integers equal, total_DE to the bit (the same rows through the same scorer in the same sub-batches)"""
    from salsa_amd.crnn.fit import validate
    from salsa_amd.crnn.train import Trainer
    tr = Trainer('cuda', seed=11)
    val_bank = bank_from_files(tmp_path, 3, 9)
    rng = np.random.RandomState(4)
    gt = [[(f, int(rng.randint(12)), int(rng.randint(-180, 180)), int(rng.randint(-40, 40)), 0) for f in range(0, FRAMES // 8, 2)] for _ in range(3)]
    forwards, plain_infer = [0], tr.infer

    def counting(x):
        forwards[0] += x.shape[0]
        return plain_infer(x)
    tr.infer = counting
    kw = dict(chunk_len=CHUNK, chunk_hop_len=HOP, eval_version='2022', sub_batch=2)
    cal = validate(tr, val_bank, gt, calibrate=CANDIDATES, **kw)
    assert forwards[0] == 3 * 3                                                                   # ONE pass: 3 clips x 3 chunks
    chosen = cal['thresholds']
    assert chosen.shape == (12,) and (chosen == cal['sweep'].best(default=0.3)[0]).all()
    plain = validate(tr, val_bank, gt, sed_threshold=chosen, **kw)
    assert {k: cal[k] for k in FIGURES} == {k: plain[k] for k in FIGURES}
    rec, rec_plain = cal['scorer'].file_records(), plain['scorer'].file_records()
    assert all((rec[k] == rec_plain[k]).all() for k in rec)
    for k in range(4):                                                                           # the sweep's records: a plain pass per candidate
        at_k = validate(tr, val_bank, gt, sed_threshold=float(CANDIDATES[k]), **kw)['scorer'].file_records()
        assert (cal['sweep'].counters[:, k, :, 0] == at_k['TP']).all() and (cal['sweep'].counters[:, k, :, 5] == at_k['DE_TP']).all()
        assert (np.abs(cal['sweep'].total_DE[:, k] - at_k['total_DE']) <= at_k['DE_TP'] * margin()).all()
