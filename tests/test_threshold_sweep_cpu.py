"""CPU tests of per-class SED thresholds and their calibration: the vector form of sed_threshold in the host
decoders, crnn/calibrate.py's host twin against a brute-force reference (tests/sweep_reference.py), the device statements of
salsa_amd/csrc/seld_sweep.h built with g++ (tests/hostemu/sweep_emu.cpp) against the host twin, the selection rule, and
validate(calibrate=) / fit(calibrate=) on a CPU trainer.

Bounds.  sweep_host against the brute force: integers equal, total_DE bit-equal (the same numpy arithmetic in the same order).  The
header against sweep_host: the status array EQUAL to what numpy's own distances say (sweep_reference.expected_status), the integers
of status-0 entries equal, a status-0 total_DE[c] within DE_TP[c] x margin (the bound tests/test_seld_score2022_gpu.py uses: the
header adds a class's slot averages per segment and then the segments, the host in one running sum, and the C library's acos is not
numpy's bit for bit -- both far below margin / DE_TP per slot)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import sweep_reference as ref
from conftest import ROOT


def margin():
    from salsa_amd.crnn.score import DEFAULT_MARGIN
    return DEFAULT_MARGIN


# ------------------------------------------------------------------------------------------------------- vector thresholds
@pytest.mark.parametrize('fmt', ['reg_xyz', 'multi_accdoa'])
def test_vector_threshold_rows_are_the_scalar_rows_class_by_class(fmt):
    case = ref.planted_case(fmt)
    vec = np.array([0.2, 0.5, 0.3])
    for f in range(ref.N_FILES):
        got = ref.host_rows(case['act'][f], case['xyz'][f], vec, ref.N_FRAMES, ref.C, fmt, 15.0)
        assert got == ref.rows_at(case['act'][f], case['xyz'][f], vec, ref.N_FRAMES, ref.C, fmt, 15.0) and len(got) > 20
        for same in (0.3, 0.5):                                            # equal entries: the scalar call's rows, bit for bit
            want = ref.host_rows(case['act'][f], case['xyz'][f], same, ref.N_FRAMES, ref.C, fmt, 15.0)
            for form in ([same] * ref.C, np.full(ref.C, same), np.full(ref.C, same, np.float32), tuple([same] * ref.C)):
                assert ref.host_rows(case['act'][f], case['xyz'][f], form, ref.N_FRAMES, ref.C, fmt, 15.0) == want


def test_float64_vector_compares_as_float32_and_nan_or_wrong_length():
    from salsa_amd.crnn.postprocess import class_thresholds, multi_accdoa_cells, multi_accdoa_rows, to_dcase_rows
    act = np.full((2, 3), np.float32(0.3))                                 # exactly float32(0.3): below the float64 0.3 ...
    act[1, 1] = np.nan
    assert float(np.float32(0.3)) > 0.3 and not (act.astype(np.float64)[0, 0] >= np.float64(0.30000002))
    xyz = np.tile(np.float32([1, 0, 0]).repeat(3), (2, 1))
    rows = to_dcase_rows(act, xyz, sed_threshold=np.array([0.3, 0.3, 0.3], np.float64), n_classes=3, max_nframes_per_file=2, eval_version='2020')
    assert rows == to_dcase_rows(act, xyz, sed_threshold=0.3, n_classes=3, max_nframes_per_file=2, eval_version='2020')
    assert [r[:2] for r in rows] == [[0, 0], [0, 1], [0, 2], [1, 0], [1, 2]]                    # ... yet active; the NaN activity is not
    nan_thr = to_dcase_rows(act, xyz, sed_threshold=[0.3, np.nan, 0.1], n_classes=3, max_nframes_per_file=2, eval_version='2020')
    assert [r[:2] for r in nan_thr] == [[0, 0], [0, 2], [1, 0], [1, 2]]                          # a NaN threshold: the class is inactive
    m_act, m_xyz = np.tile(act, (1, 3)), np.tile(np.float32([1, 0, 0]).repeat(9), (2, 1))        # three equal tracks (1, 0, 0) per class
    m_rows = multi_accdoa_rows(m_act, m_xyz, sed_threshold=np.array([0.3, np.nan, 0.3]), n_classes=3, max_nframes_per_file=2, eval_version='2020')
    assert [r[:2] for r in m_rows] == [[0, 0], [0, 2], [1, 0], [1, 2]]                           # (three equal tracks unify into one row)
    assert class_thresholds(0.3, 3).shape == () and class_thresholds([0.3] * 3, 3).dtype == np.float32
    for bad in ([0.3, 0.3], [0.3] * 4, [[0.3] * 3], []):
        with pytest.raises(ValueError, match='sed_threshold'):
            to_dcase_rows(act, xyz, sed_threshold=bad, n_classes=3, max_nframes_per_file=2)
        with pytest.raises(ValueError, match='sed_threshold'):
            multi_accdoa_cells(m_act, m_xyz, bad, 0.9, 3)
        with pytest.raises(ValueError, match='sed_threshold'):
            multi_accdoa_rows(m_act, m_xyz, sed_threshold=bad, n_classes=3, max_nframes_per_file=2)


def test_a_wrong_length_is_refused_before_any_device_call():
    """decode._device_thresholds raises on the host: nothing is launched (these are CPU tensors, which the wrappers refuse LATER)"""
    from salsa_amd.crnn.decode import _device_thresholds
    assert _device_thresholds(0.3, 3, 'cpu') is None
    t = _device_thresholds(np.array([0.1, 0.2, 0.3]), 3, 'cpu')
    assert t.dtype == torch.float32 and t.tolist() == [float(np.float32(v)) for v in (0.1, 0.2, 0.3)]
    with pytest.raises(ValueError, match='sed_threshold'):
        _device_thresholds([0.1, 0.2], 3, 'cpu')


# ------------------------------------------------------------------------------------------------------- the host twin
@pytest.fixture(scope='module', params=['reg_xyz', 'multi_accdoa'])
def planted(request):
    from salsa_amd.crnn.calibrate import sweep_host
    case = ref.planted_case(request.param)
    host = sweep_host(case['act'], case['xyz'], case['gt'], case['thresholds'], n_frames=ref.N_FRAMES, n_classes=ref.C,
                      doa_threshold=ref.DOA_THRESHOLD, label_rate=ref.RATE, output_format=case['fmt'], unify_deg=case['unify_deg'])
    return case, host


def test_sweep_host_equals_the_brute_force(planted):
    case, host = planted
    counters, de = ref.brute_force(case['act'], case['xyz'], case['gt'], case['thresholds'], ref.N_FRAMES, ref.C, case['fmt'], case['unify_deg'])
    assert host.counters.shape == (3, 6, 3, 8) and host.counters.dtype == np.int64 and host.total_DE.shape == (3, 6, 3)
    assert (host.counters == counters).all() and host.total_DE.tobytes() == de.tobytes()
    TP, FP, FPs, FN, Nref, DE_TP = (host.counters[..., k] for k in range(6))
    assert TP.sum() > 20 and FPs.sum() > 10 and FN.sum() > 10 and FP.sum() > 0                    # the case exercises every counter
    assert (Nref == Nref[:, :1]).all()                                                           # the references do not depend on k
    assert (DE_TP[:, 0, :2] >= DE_TP[:, 5, :2]).all() and not DE_TP[:, 5, :2].any()              # above every activity: nothing predicted
    if case['fmt'] == 'multi_accdoa':                                                            # file 2, frame 1, class 1: unified at 0.3, not at 0.5
        rows = {t: [r for r in ref.host_rows(case['act'][2], case['xyz'][2], t, ref.N_FRAMES, ref.C, 'multi_accdoa', 15.0) if r[:2] == [1, 1]]
                for t in (0.3, 0.5)}
        assert [r[2:] for r in rows[0.3]] == [[42, 10]] or [r[2:] for r in rows[0.3]] == [[43, 10]]
        assert [r[2:] for r in rows[0.5]] == [[40, 10]]


def test_sweep_host_accumulates_and_merges():
    from salsa_amd.crnn.calibrate import ThresholdSweep, sweep_host
    case = ref.planted_case('reg_xyz')
    kw = dict(n_frames=ref.N_FRAMES, n_classes=ref.C, label_rate=ref.RATE)
    whole = sweep_host(case['act'], case['xyz'], case['gt'], case['thresholds'], **kw)
    acc = ThresholdSweep(case['thresholds'], ref.C, 20, ref.RATE)
    for lo, hi in ((0, 2), (2, 3)):
        assert sweep_host(case['act'][lo:hi], case['xyz'][lo:hi], case['gt'][lo:hi], None, accumulator=acc, **kw) is acc
    assert (acc.counters == whole.counters).all() and acc.total_DE.tobytes() == whole.total_DE.tobytes()
    other = ThresholdSweep(case['thresholds'], ref.C, 20, ref.RATE).merge(whole).merge(whole)
    assert other.counters.shape[0] == 6 and (other.counters[3:] == whole.counters).all()
    one_grid = ThresholdSweep(ref.GRID, ref.C)
    assert one_grid.thresholds.shape == (6, 3) and one_grid.thresholds.dtype == np.float32 and (one_grid.thresholds == ref.GRID[:, None]).all()
    for bad in (ThresholdSweep(ref.GRID, ref.C), ThresholdSweep(case['thresholds'], ref.C, 30), object()):
        with pytest.raises(ValueError, match='merge'):
            acc.merge(bad)
    for bad in (np.zeros((65,)), np.zeros((0,)), np.zeros((4, 2)), np.zeros((2, 3, 3)), 0.3):
        with pytest.raises(ValueError, match='thresholds'):
            ThresholdSweep(bad, 3)


# ------------------------------------------------------------------------------------------------------- the header
@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('sweep_emu') / 'libsweep_emu.so')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-fno-builtin-sin', '-fno-builtin-cos', '-o', so,
                           os.path.join(ROOT, 'tests', 'hostemu', 'sweep_emu.cpp')])
    L = C.CDLL(so)
    fp, sp, ip, dp = C.POINTER(C.c_float), C.POINTER(C.c_int16), C.POINTER(C.c_int), C.POINTER(C.c_double)
    L.emu_sweep_file.argtypes = [fp, fp, C.c_int, C.c_int, C.c_int, C.c_double, fp, C.c_int, sp, C.c_int, C.c_int, C.c_double, C.c_double, ip, dp, ip]
    return L


def emu_sweep(emu, act, xyz, gt, thresholds, n_frames, n_classes, fmt, unify_deg, rate=ref.RATE):
    """-> five (files, n_seg, K, C, 5), class_de (files, n_seg, K, C), status (files, n_seg, K, C); pre-filled: an element left out shows"""
    from salsa_amd.crnn.postprocess import cos_unify_of
    from salsa_amd.crnn.score import pack_rows
    rows, counts = pack_rows(gt)
    n, n_seg, K = len(act), -(-n_frames // rate), thresholds.shape[0]
    five, status = np.full((n, n_seg, K, n_classes, 5), -7, np.int32), np.full((n, n_seg, K, n_classes), -7, np.int32)
    de = np.full((n, n_seg, K, n_classes), np.nan)
    fp, sp, ip, dp = C.POINTER(C.c_float), C.POINTER(C.c_int16), C.POINTER(C.c_int), C.POINTER(C.c_double)
    thr = np.ascontiguousarray(thresholds, np.float32)
    for f in range(n):
        a, x, g = np.ascontiguousarray(act[f], np.float32), np.ascontiguousarray(xyz[f], np.float32), np.ascontiguousarray(rows[f])
        emu.emu_sweep_file(a.ctypes.data_as(fp), x.ctypes.data_as(fp), n_frames, n_classes, int(fmt == 'multi_accdoa'), cos_unify_of(unify_deg),
                           thr.ctypes.data_as(fp), K, g.ctypes.data_as(sp), int(counts[f]), rate, float(ref.DOA_THRESHOLD), margin(),
                           five[f].ctypes.data_as(ip), de[f].ctypes.data_as(dp), status[f].ctypes.data_as(ip))
    assert (five >= 0).all() and (status >= 0).all() and not np.isnan(de).any()
    return five, de, status


def check_against_host(five, de, status, host, want_status):
    """the device-side records (emulated or real) of a case against its sweep_host result"""
    from salsa_amd.crnn.calibrate import _eight
    assert (status == want_status).all()
    assert not five[status != 0].any() and not de[status != 0].any()                             # doubt / refused entries carry zeros
    clean = (want_status == 0).all(axis=1)                                                       # (files, K, C): no segment went to the host
    got, got_de = _eight(five.astype(np.int64)).sum(axis=1), de.sum(axis=1)
    assert clean.any() and (got[clean] == host.counters[clean]).all()
    assert (np.abs(got_de - host.total_DE)[clean] <= host.counters[..., 5][clean] * margin()).all()
    return clean


def test_header_equals_sweep_host_on_the_planted_case(emu, planted):
    case, host = planted
    five, de, status = emu_sweep(emu, case['act'], case['xyz'], case['gt'], case['thresholds'], ref.N_FRAMES, ref.C, case['fmt'], case['unify_deg'])
    want = ref.expected_status(case['act'], case['xyz'], case['gt'], case['thresholds'], ref.N_FRAMES, ref.C, case['fmt'], case['unify_deg'], margin())
    check_against_host(five, de, status, host, want)
    # the planted entries, counted exactly: the 20-degree slot wherever frame 2 of file 1 is active for class 2 (0.6 >= the candidate:
    # k = 1 .. 4 of the shifted column), five references in file 1, segment 1, class 0 at every candidate -- and nothing else
    assert (np.argwhere(status == 1) == [[1, 0, k, 2] for k in (1, 2, 3, 4)]).all() and (status == 1).sum() == 4
    assert (np.argwhere(status == 2) == [[1, 1, k, 0] for k in range(6)]).all() and (status == 2).sum() == 6
    assert (host.counters[0, :, 0, 4] >= 2).all()                                                # two references of class 0 in file 0, frame 6


@pytest.mark.parametrize('fmt,n_classes,rate,K', [('reg_xyz', 32, 10, 64), ('multi_accdoa', 32, 32, 8), ('multi_accdoa', 13, 10, 3),
                                                  ('reg_xyz', 32, 32, 2)])
def test_header_at_the_limits_and_across_class_groups(emu, fmt, n_classes, rate, K):
    """32 classes x 64 candidates, and the shapes at which the classes no longer fit one group of entries (multi at rate 32: groups
    of 4; single-vector 32 x 32: 30 + 2) or just fit (13 classes of Multi-ACCDOA at rate 10)"""
    from salsa_amd.crnn.calibrate import sweep_host
    n_frames = 2 * rate + 3
    act, xyz, gt = ref.random_case(5, 1, n_frames, n_classes, fmt, gt_density=0.3)
    thresholds = np.linspace(0.05, 1.0, K * n_classes, dtype=np.float32).reshape(n_classes, K).T.copy()     # every (k, c) its own value
    host = sweep_host(act, xyz, gt, thresholds, n_frames=n_frames, n_classes=n_classes, label_rate=rate, output_format=fmt)
    five, de, status = emu_sweep(emu, act, xyz, gt, thresholds, n_frames, n_classes, fmt, 15.0, rate)
    want = ref.expected_status(act, xyz, gt, thresholds, n_frames, n_classes, fmt, 15.0, margin(), label_rate=rate)
    assert (want != 0).mean() <= 0.02
    clean = check_against_host(five, de, status, host, want)
    assert clean.mean() > 0.9 and host.counters[..., 0].sum() > 0


def test_seeded_random_case_has_few_doubts():
    """the seed of the GPU suite's random case (2 files x 600 x 12, K = 17), checked here with angular_distance_deg on the host rows:
    at most 2 % of the entries may be doubt"""
    act, xyz, gt = ref.random_case(ref.RANDOM_SEED, 2, 600, 12, 'reg_xyz')
    thresholds = np.repeat(np.linspace(0.1, 0.9, 17, dtype=np.float32)[:, None], 12, axis=1)
    want = ref.expected_status(act, xyz, gt, thresholds, 600, 12, 'reg_xyz', 15.0, margin())
    assert (want != 0).mean() <= 0.02 and (want == 0).any()


# ------------------------------------------------------------------------------------------------------- the selection rule
def planted_sweep(TP, FN, de, thresholds, nref=None):
    """a sweep of one file whose class c at candidate k has TP[k][c] hits at total error de[k][c] and FN[k][c] misses"""
    from salsa_amd.crnn.calibrate import ThresholdSweep
    TP, FN, de = np.asarray(TP, np.int64), np.asarray(FN, np.int64), np.asarray(de, np.float64)
    K, n = TP.shape
    s = ThresholdSweep(thresholds, n)
    cnt = np.zeros((1, K, n, 8), np.int64)
    cnt[0, :, :, 0], cnt[0, :, :, 3], cnt[0, :, :, 7] = TP, FN, FN
    cnt[0, :, :, 5] = TP
    cnt[0, :, :, 4] = (TP + FN) if nref is None else nref
    return s.add_files(cnt, de[None])


def test_best_picks_the_least_J_breaks_ties_upward_and_falls_back_to_the_default():
    # class 0: a clear winner at k = 1; class 1: k = 0 and k = 2 tie exactly -- the greater value (k = 2) wins; class 2: equal values
    # at k = 1, 2 tie -- the lower index; class 3: no reference anywhere -> the default
    TP = [[2, 3, 1, 0], [4, 1, 2, 0], [1, 3, 2, 0]]
    FN = [[2, 1, 3, 0], [0, 3, 2, 0], [3, 1, 2, 0]]
    de = [[10., 30., 5., 0.], [20., 10., 14., 0.], [5., 30., 14., 0.]]
    thr = np.array([[0.2, 0.2, 0.2, 0.2], [0.4, 0.4, 0.5, 0.4], [0.6, 0.6, 0.5, 0.6]], np.float32)
    s = planted_sweep(TP, FN, de, thr)
    cw = s.classwise()
    assert cw.shape == (3, 4, 4)
    from salsa_amd.crnn.metrics import SeldMetrics2022
    for k in range(3):
        want = SeldMetrics2022._classwise(s.counters[0, k], s.total_DE[0, k], np.zeros(3, np.int64))
        assert (cw[k, :, :3] == want[:, 1:4]).all()
        assert (cw[k, :, 3] == ((1 - want[:, 1]) + want[:, 2] / 180 + (1 - want[:, 3])) / 3).all()
    assert cw[0, 1, 3] == cw[2, 1, 3] < cw[1, 1, 3] and cw[1, 2, 3] == cw[2, 2, 3] < cw[0, 2, 3] and cw[1, 0, 3] < min(cw[0, 0, 3], cw[2, 0, 3])
    chosen, index = s.best(default=0.35)
    assert chosen.dtype == np.float32 and index.tolist() == [1, 2, 1, -1]
    assert chosen.tolist() == [float(np.float32(v)) for v in (0.4, 0.6, 0.5, 0.35)]
    assert s.best()[0][3] == np.float32(0.3) and s.best(default=[0.1, 0.2, 0.3, 0.45])[0][3] == np.float32(0.45)
    flipped = planted_sweep(TP[::-1], FN[::-1], de[::-1], thr[::-1])                             # the tie goes to the greater VALUE, not the later index
    assert flipped.best()[1].tolist() == [1, 0, 0, -1] and (flipped.best()[0][:3] == chosen[:3]).all()


# ------------------------------------------------------------------------------------------------------- validate and fit
F, CHUNK, FRAMES = 32, 64, 128
CANDIDATES = np.array([0.3, 0.45, 0.5, 0.55], np.float32)


def make_bank(n_clips, nc=12, seed=0, hop=32):
    from salsa_amd.dataset import GpuFeatureBank
    g = torch.Generator().manual_seed(seed)
    bank = GpuFeatureBank(None, chunk_len_s=CHUNK / 80, chunk_hop_len_s=hop / 80, n_classes=nc, device='cpu')
    feats = torch.randn(n_clips, 7, FRAMES, F, generator=g)
    sed = (torch.rand(n_clips, FRAMES // 8, nc, generator=g) < 0.2).float()
    v = torch.randn(n_clips, FRAMES // 8, 3, nc, generator=g)
    doa = ((v / v.norm(dim=2, keepdim=True)) * sed[:, :, None, :]).reshape(n_clips, FRAMES // 8, 3 * nc)
    bank.add_features(feats, ['clip%d' % i for i in range(n_clips)], sed=sed.numpy(), doa=doa.numpy())
    return bank.finalize(normalize=False)


def make_gt(n_clips, nc=12):
    rng = np.random.RandomState(4)
    return [[(int(f), int(rng.randint(nc)), float(rng.randint(-180, 180)), float(rng.randint(-40, 40)), 0) for f in range(0, FRAMES // 8, 2)]
            for _ in range(n_clips)]


FIGURES = ('valER', 'valF1', 'valLE', 'valLR', 'valSeld')


def test_validate_calibrate_equals_validate_at_the_chosen_vector():
    from salsa_amd.crnn.calibrate import ThresholdSweep
    from salsa_amd.crnn.fit import validate
    from salsa_amd.crnn.train import Trainer
    tr = Trainer('cpu', amp_dtype=None, seed=11)
    val_bank, gt = make_bank(3, seed=9), make_gt(3)
    forwards = [0]
    plain_infer = tr.infer

    def counting(x):
        forwards[0] += x.shape[0]
        return plain_infer(x)
    tr.infer = counting
    kw = dict(chunk_len=CHUNK, chunk_hop_len=32, eval_version='2022', sub_batch=2)
    cal = validate(tr, val_bank, gt, calibrate=CANDIDATES, **kw)
    assert forwards[0] == 3 * 3                                                                   # ONE pass: 3 clips x 3 chunks
    chosen, sweep = cal['thresholds'], cal['sweep']
    assert isinstance(sweep, ThresholdSweep) and sweep.counters.shape == (3, 4, 12, 8) and sweep.outputs == []
    assert chosen.dtype == np.float32 and chosen.shape == (12,) and (chosen == sweep.best(default=0.3)[0]).all()
    assert set(np.unique(chosen)) <= set(CANDIDATES.tolist()) | {np.float32(0.3)}
    plain = validate(tr, val_bank, gt, sed_threshold=chosen, return_rows=True, **kw)
    assert {k: cal[k] for k in FIGURES} == {k: plain[k] for k in FIGURES}
    rec, rec_plain = cal['scorer'].file_records(), plain['scorer'].file_records()
    assert all((rec[k] == rec_plain[k]).all() for k in rec)
    # the sweep's own records are sweep_host's on the combined outputs, which the rows of the plain pass were decoded from
    for k in range(4):
        at_k = validate(tr, val_bank, gt, sed_threshold=float(CANDIDATES[k]), **kw)['scorer'].file_records()
        assert (sweep.counters[:, k, :, 0] == at_k['TP']).all() and (sweep.total_DE[:, k] == at_k['total_DE']).all()
    # the trainer's calibrated vector is the default of later calls; without it the default stays 0.3
    assert {k: validate(tr, val_bank, gt, **kw)[k] for k in FIGURES} == {k: validate(tr, val_bank, gt, sed_threshold=0.3, **kw)[k] for k in FIGURES}
    tr.sed_thresholds = chosen
    assert {k: validate(tr, val_bank, gt, **kw)[k] for k in FIGURES} == {k: plain[k] for k in FIGURES}
    for version in ('2020', '2021'):
        with pytest.raises(ValueError, match="eval_version='2022'"):
            validate(tr, val_bank, gt, calibrate=CANDIDATES, eval_version=version)


def test_fit_calibrate_stores_and_restores_the_thresholds(tmp_path):
    from salsa_amd.crnn.train import Trainer
    bank, val_bank, gt = make_bank(2), make_bank(2, seed=9), make_gt(2)
    kw = dict(val_bank=val_bank, val_gt=gt, batch_size=3, max_epochs=2, seed=5, audio_format='foa', eval_version='2022',
              milestones=(0.0, 0.1, 0.7, 1.0), lrs=(3e-4, 3e-4, 3e-4, 1e-4), moms=(0.95, 0.85, 0.9, 0.99), val_interval=1)
    plain = Trainer('cpu', amp_dtype=None, seed=11)
    h_plain = plain.fit(bank, out_dir=str(tmp_path / 'plain'), **kw)
    again = Trainer('cpu', amp_dtype=None, seed=11)
    h_none = again.fit(bank, out_dir=str(tmp_path / 'none'), calibrate=None, **kw)
    assert h_none == h_plain and again.sed_thresholds is None                                    # calibrate=None: the parent's history
    ckpt = torch.load(str(tmp_path / 'none' / 'checkpoint' / 'epoch=001.ckpt'), weights_only=False)
    assert 'sed_thresholds' not in ckpt and all(set(v) == set(FIGURES) | {'epoch'} for v in h_none['val'])
    cal = Trainer('cpu', amp_dtype=None, seed=11)
    h_cal = cal.fit(bank, out_dir=str(tmp_path / 'cal'), calibrate=CANDIDATES, **kw)
    assert h_cal['steps'] == h_plain['steps']                                                    # training is untouched
    assert all(set(v) == set(FIGURES) | {'epoch', 'thresholds'} and len(v['thresholds']) == 12 for v in h_cal['val'])
    assert cal.sed_thresholds.dtype == np.float32 and cal.sed_thresholds.tolist() == h_cal['val'][-1]['thresholds']
    assert h_cal['best']['valSeld'] == min(v['valSeld'] for v in h_cal['val'])                   # the best checkpoint: by the calibrated figure
    from salsa_amd.crnn.fit import validate
    at = validate(cal, val_bank, gt, sed_threshold=cal.sed_thresholds, eval_version='2022')
    assert {k: at[k] for k in FIGURES} == {k: h_cal['val'][-1][k] for k in FIGURES}
    for d in ('checkpoint', 'best'):
        name = os.listdir(str(tmp_path / 'cal' / d))[0]
        ckpt = torch.load(str(tmp_path / 'cal' / d / name), weights_only=False)
        epoch_val = [v for v in h_cal['val'] if v['epoch'] == ckpt['epoch']][0]
        assert ckpt['sed_thresholds'].dtype == np.float32 and ckpt['sed_thresholds'].tolist() == epoch_val['thresholds']
    # resume restores them (one more epoch is asked for, none is left: only the load happens) ...
    resumed = Trainer('cpu', amp_dtype=None, seed=77)
    assert resumed.sed_thresholds is None
    h_res = resumed.fit(bank, out_dir=str(tmp_path / 'cal'), calibrate=CANDIDATES, resume=True, **kw)
    assert h_res == h_cal and (resumed.sed_thresholds == cal.sed_thresholds).all()
    # ... and a checkpoint without the key resumes as before
    old = Trainer('cpu', amp_dtype=None, seed=77)
    assert old.fit(bank, out_dir=str(tmp_path / 'plain'), resume=True, **kw) == h_plain and old.sed_thresholds is None
    for version in ('2020', '2021'):
        with pytest.raises(ValueError, match="eval_version='2022'"):
            old.fit(bank, **dict(kw, eval_version=version, calibrate=CANDIDATES))


def test_infer_pipelined_sweep_on_the_host_with_and_without_rows():
    """decode='host' with a stub forward: the sweep is sweep_host on the combined outputs it keeps, the rows are those of the call
    without sweep=, return_rows=False builds none, and a per-class sed_threshold of the wrong length is refused before any forward"""
    from salsa_amd.crnn.calibrate import ThresholdSweep, sweep_host
    from salsa_amd.crnn.infer import infer_pipelined
    case = ref.planted_case('reg_xyz')
    act, xyz = torch.from_numpy(case['act']), torch.from_numpy(case['xyz'])
    calls = [0]

    def forward(x):
        calls[0] += 1
        lo = int(x[0, 0, 0, 0])
        return act[lo:lo + x.shape[0]], xyz[lo:lo + x.shape[0]]
    featurize = lambda lo, hi: torch.arange(lo, hi, dtype=torch.float32).reshape(-1, 1, 1, 1)      # noqa: E731
    kw = dict(sub_batch=2, sed_threshold=[0.3, 0.5, 0.2], n_label_frames=ref.N_FRAMES, n_classes=ref.C, eval_version='2020', decode='host')
    acc = ThresholdSweep(case['thresholds'], ref.C, 20, ref.RATE)
    rows = infer_pipelined(3, featurize, forward, sweep=(case['gt'], None, acc), **kw)
    assert rows == infer_pipelined(3, featurize, forward, **kw) and sum(map(len, rows)) > 0
    host = sweep_host(case['act'], case['xyz'], case['gt'], case['thresholds'], n_frames=ref.N_FRAMES, n_classes=ref.C, label_rate=ref.RATE)
    assert (acc.counters == host.counters).all() and acc.total_DE.tobytes() == host.total_DE.tobytes()
    assert [a.shape for a, _ in acc.outputs] == [(2, ref.N_FRAMES, ref.C), (1, ref.N_FRAMES, ref.C)]
    quiet = ThresholdSweep(case['thresholds'], ref.C, 20, ref.RATE)
    assert infer_pipelined(3, featurize, forward, sweep=(case['gt'], None, quiet), return_rows=False, **kw) == [None] * 3
    assert (quiet.counters == host.counters).all() and quiet.total_DE.tobytes() == host.total_DE.tobytes()
    before = calls[0]
    with pytest.raises(ValueError, match='sed_threshold'):
        infer_pipelined(3, featurize, forward, **dict(kw, sed_threshold=[0.3, 0.5]))
    assert calls[0] == before


# ------------------------------------------------------------------------------------------------------- the exports
@pytest.fixture(scope='module')
def lib():
    from salsa_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_exports_are_declared_and_share_the_existing_sources():
    from salsa_amd import _lib
    i, f, d, vp = C.c_int, C.c_float, C.c_double, C.c_void_p
    P = _lib.PROTOTYPES['salsa_nn.h']
    assert P['salsa_nn_seld_decode'] == (i, [vp, vp, i, i, i, i, i, i, f, i, vp, vp, vp, vp, vp])      # the old entries keep their signatures
    assert P['salsa_nn_seld_decode_thr'] == (i, [vp, vp, i, i, i, i, i, i, vp, i, vp, vp, vp, vp, vp])
    assert P['salsa_nn_seld_decode_multi'] == (i, [vp, vp, i, i, i, i, f, d, vp, vp, vp])
    assert P['salsa_nn_seld_decode_multi_thr'] == (i, [vp, vp, i, i, i, i, vp, d, vp, vp, vp])
    assert P['salsa_nn_seld_sweep'] == (i, [vp, vp, i, i, i, i, i, d, vp, i, vp, vp, i, i, d, d, vp, vp, vp, vp, vp, vp])
    csrc = os.path.join(ROOT, 'salsa_amd', 'csrc')
    assert os.path.join(csrc, 'seld_sweep.hip') in _lib.build_command()
    src, hdr = open(os.path.join(csrc, 'seld_sweep.hip')).read(), open(os.path.join(csrc, 'seld_sweep.h')).read()
    assert '#include "seld_sweep.h"' in src and '#include "build_guard.h"' in src and 'atomic' not in src.split('#include', 1)[1]
    for shared in ('#include "seld_score.h"', '#include "seld_decode.h"', '#include "multi_accdoa.h"', 'unify_cell(', 'pair_cell(', 'xyz_to_angles(',
                   'score_class_sel(', 'class_record2022(', 'is_active('):
        assert shared in hdr, shared
    assert '#include "../../salsa_amd/csrc/seld_sweep.h"' in open(os.path.join(ROOT, 'tests', 'hostemu', 'sweep_emu.cpp')).read()


def test_launchers_refuse_bad_arguments_before_any_device_call(lib):
    """every call returns E_INVAL from the host-side checks: nothing is launched, no pointer is read (they point nowhere)"""
    from salsa_amd import _lib
    names = ('act', 'xyz', 'thresholds', 'gt_rows', 'gt_counts', 'class_counters', 'class_de', 'status', 'file_counters', 'file_de')
    p = {k: C.c_void_p(0x1000 * (i + 1)) for i, k in enumerate(names)}
    good = dict(n_files=4, n_in=600, n_frames=600, n_classes=12, multi=1, cos=0.96, K=17, cap=900, rate=10, thr=20.0, margin=1e-4, **p)

    def call(**kw):
        a = dict(good, **kw)
        return lib.salsa_nn_seld_sweep(a['act'], a['xyz'], a['n_files'], a['n_in'], a['n_frames'], a['n_classes'], a['multi'], a['cos'], a['thresholds'],
                                       a['K'], a['gt_rows'], a['gt_counts'], a['cap'], a['rate'], a['thr'], a['margin'], a['class_counters'],
                                       a['class_de'], a['status'], a['file_counters'], a['file_de'], None)
    for k in names:
        assert call(**{k: None}) == _lib.E_INVAL and 'salsa_nn_seld_sweep' in _lib.last_error(), k   # (the file sums: both or neither)
    for k in ('gt_rows', 'class_de', 'file_counters', 'file_de'):
        assert call(**{k: C.c_void_p(0x1004)}) == _lib.E_INVAL and 'misaligned' in _lib.last_error(), k
    for k in ('act', 'xyz', 'thresholds', 'status'):
        assert call(**{k: C.c_void_p(0x1002)}) == _lib.E_INVAL, k
    for k, bad in (('n_classes', (0, -1, 33)), ('rate', (0, -10, 33)), ('K', (0, -1, 65)), ('n_files', (0, 65536)), ('n_frames', (0, 32768)),
                   ('n_in', (599, 32768)), ('cap', (0, -1)), ('multi', (-1, 2)), ('cos', (float('nan'), 1.5, -1.5)),
                   ('margin', (-1e-9, float('nan'), float('inf'))), ('thr', (float('nan'),))):
        for v in bad:
            assert call(**{k: v}) == _lib.E_INVAL, (k, v)
    q = {k: C.c_void_p(0x1000 * (i + 1)) for i, k in enumerate(('a', 'x', 'thr', 'rows', 'counts'))}
    assert lib.salsa_nn_seld_decode_thr(q['a'], q['x'], 2, 1, 60, 60, 60, 12, None, 0, q['rows'], q['counts'], None, None, None) == _lib.E_INVAL
    assert lib.salsa_nn_seld_decode_thr(q['a'], q['x'], 2, 1, 60, 60, 60, 12, C.c_void_p(0x1002), 0, q['rows'], q['counts'], None, None, None) == _lib.E_INVAL
    assert lib.salsa_nn_seld_decode_thr(q['a'], q['x'], 2, 2, 60, 60, 60, 12, q['thr'], 0, q['rows'], q['counts'], None, None, None) == _lib.E_INVAL
    assert lib.salsa_nn_seld_decode_multi_thr(q['a'], q['x'], 2, 60, 60, 12, None, 0.96, q['rows'], q['counts'], None) == _lib.E_INVAL
    assert lib.salsa_nn_seld_decode_multi_thr(q['a'], q['x'], 2, 50, 60, 12, q['thr'], 0.96, q['rows'], q['counts'], None) == _lib.E_INVAL
