"""CPU tests of the device scorer's class-wise SELD 2022 statements (salsa_amd/csrc/seld_score.h built with g++:
tests/hostemu/score2022_emu.cpp) against crnn/metrics.py::SeldMetrics2022, of the 2022 side of crnn/score.py, of the export and of the
launcher's argument checks.

Bounds.  The per-segment class counters, S, D, I and the status are EQUAL to SeldMetrics2022 run on the segment alone (status: as
numpy's own costs say, seld_score_cases.expected_status).  A class's share of total_DE is held within DE_TP[c] x margin / 20: the
emulation calls the C library's sin / cos / acos, numpy's arccos is not the C library's on every machine (at most 7.2e-13 degrees per
distance, tests/test_seld_score_cpu.py), and margin / 20 = 5e-6 degrees per slot average is far above that and 20 times below what
would move a decision -- in practice the two agree to rounding.  After resolve_records every integer counter and every FILE record is
equal to the host scorer's."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import seld_score_cases as cases
import seld_score2022_cases as cases22
from conftest import ROOT


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('score2022_emu') / 'libscore2022_emu.so')
    # -fno-builtin-sin / -cos: g++ otherwise merges sin(e) and cos(e) into one sincos call, whose results are not always sin's and cos's
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-fno-builtin-sin', '-fno-builtin-cos', '-o', so,
                           os.path.join(ROOT, 'tests', 'hostemu', 'score2022_emu.cpp')])
    L = C.CDLL(so)
    sp, ip, dp = C.POINTER(C.c_int16), C.POINTER(C.c_int), C.POINTER(C.c_double)
    L.emu_score2022_file.argtypes = [sp, C.c_int, sp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, ip, dp, ip, ip]
    return L


def margin():
    from salsa_amd.crnn.score import DEFAULT_MARGIN
    return DEFAULT_MARGIN


def emu_records(emu, pred_files, gt_files, kw, margin):
    """-> class counters (files, n_seg, C, 5), class total_DE (files, n_seg, C), sdi (files, n_seg, 3), status (files, n_seg) of the
    emulation, through score.pack_rows; every output pre-filled, so an element the statements leave out shows"""
    from salsa_amd.crnn.score import pack_rows
    (pr, pc), (gr, gc) = pack_rows(pred_files), pack_rows(gt_files)
    n, n_seg, nc = len(pred_files), -(-kw['n_frames'] // kw['label_rate']), kw['n_classes']
    five, sdi, status = (np.full(shape, -7, dtype=np.int32) for shape in ((n, n_seg, nc, 5), (n, n_seg, 3), (n, n_seg)))
    de = np.full((n, n_seg, nc), np.nan)
    sp, ip, dp = C.POINTER(C.c_int16), C.POINTER(C.c_int), C.POINTER(C.c_double)
    for f in range(n):
        p, g = np.ascontiguousarray(pr[f]), np.ascontiguousarray(gr[f])
        emu.emu_score2022_file(p.ctypes.data_as(sp), int(pc[f]), g.ctypes.data_as(sp), int(gc[f]), kw['n_frames'], kw['label_rate'], nc,
                               float(kw['doa_threshold']), margin, five[f].ctypes.data_as(ip), de[f].ctypes.data_as(dp),
                               sdi[f].ctypes.data_as(ip), status[f].ctypes.data_as(ip))
    assert (five >= 0).all() and (sdi >= 0).all() and not np.isnan(de).any()
    return five, de, sdi, status


def check_case(emu, name, pred_files, gt_files, kw, average='macro'):
    from salsa_amd.crnn.score import DeviceSeldScore2022, resolve_records
    records = emu_records(emu, pred_files, gt_files, kw, margin())
    sums = cases22.check_records(name, pred_files, gt_files, kw, margin(), records, margin() / 20)
    got = resolve_records(sums[0], sums[1], records[3], lambda f: (pred_files[f], gt_files[f]), margin=margin(), eval_version='2022',
                          sum_sdi=sums[2], average=average, **kw)
    assert isinstance(got, DeviceSeldScore2022) and got.average == average and got.eval_version == '2022'
    status = records[3]
    assert (got.n_segments, got.n_doubt, got.n_refused) == (status.size, int((status == 1).sum()), int((status == 2).sum()))
    cases22.check_result(name, got, pred_files, gt_files, kw, margin())
    return got, status


FAMILIES = cases.built_families()


@pytest.mark.parametrize('k', range(len(FAMILIES)), ids=[c[0].replace(' ', '_') for c in FAMILIES])
def test_built_family(emu, k):
    name, pred, gt, kw = FAMILIES[k]
    want = cases22.expected_statuses(pred, gt, kw, margin())
    assert (want != 0).mean() <= cases22.DOUBT_CAP, name                                   # the statements, not the host, are what is tested
    check_case(emu, name, pred, gt, kw)


SMALL = [cases22.main_case()] + cases22.edge_cases()


@pytest.mark.parametrize('k', range(len(SMALL)), ids=[c[0].replace(' ', '_') for c in SMALL])
def test_main_case_and_edges(emu, k):
    name, pred, gt, kw = SMALL[k]
    want = cases22.expected_statuses(pred, gt, kw, margin())
    assert (want != 0).mean() <= cases22.DOUBT_CAP, name
    got, status = check_case(emu, name, pred, gt, kw, average='micro' if k % 2 else 'macro')
    if name == 'main case':
        assert not status.any()
        f0 = {n: v[0] for n, v in got.file_records().items()}                              # file 0, by hand (main_case's docstring)
        assert [list(f0[n]) for n in ('TP', 'FP', 'FP_spatial', 'FN', 'Nref')] == [[1, 1, 1, 2], [0, 3, 0, 0], [1, 0, 0, 1], [1, 0, 4, 0], [3, 1, 4, 3]]
        assert (f0['S'], f0['D'], f0['I']) == (1 + 2, 2 + 0, 0 + 2) and not any(v[2].any() for v in got.file_records().values())


@pytest.mark.parametrize('k', range(2), ids=['doubt', 'refusal'])
def test_a_doubt_or_refused_segment_is_resolved_into_its_own_file(emu, k):
    name, pred, gt, kw, want = cases22.doubt_and_refusal_cases()[k]
    got, status = check_case(emu, name, pred, gt, kw)
    assert status[1, 1] == want and (np.delete(status.reshape(-1), 4) == 0).all()
    assert (got.n_doubt, got.n_refused) == ((1, 0) if want == 1 else (0, 1))
    alone = cases22.host_segment(pred[1], gt[1], 1, kw)
    assert alone[0][:, 1].sum() > 0                                                        # the segment does hold something ...
    without = cases22.host_total([pred[0], cases.segment_rows_of(pred[1], 0, 10) + cases.segment_rows_of(pred[1], 2, 10), pred[2]],
                                 [gt[0], cases.segment_rows_of(gt[1], 0, 10) + cases.segment_rows_of(gt[1], 2, 10), gt[2]], kw)
    rec, rec_without = got.file_records(), without.file_records()
    assert (rec['Nref'][[0, 2]] == rec_without['Nref'][[0, 2]]).all() and (rec['Nref'][1] == rec_without['Nref'][1] + alone[0][:, 1]).all()   # ... and it went to file 1


def test_knife_edges_go_to_the_host(emu):
    for name, pred, gt, kw in cases.knife_edges():
        _, status = check_case(emu, name, pred, gt, kw)
        assert status[:, 0].all() and not status[:, 1].any(), name


# ---------------------------------------------------------------------------------------------------- the export and its checks
def test_seld_score2022_is_declared_listed_and_built_from_the_shared_source():
    from salsa_amd import _lib
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'salsa_nn.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+salsa_nn_seld_score2022\s*\(', hdr) and 'salsa_nn_seld_score2022' in _lib.NN_EXPORTS
    i, d, vp = C.c_int, C.c_double, C.c_void_p
    assert _lib.PROTOTYPES['salsa_nn.h']['salsa_nn_seld_score2022'] == (i, [vp, vp, i, vp, vp, i, i, i, i, i, d, d, vp, vp, vp, vp, vp, vp, vp, vp])
    assert _lib.PROTOTYPES['salsa_nn.h']['salsa_nn_seld_score2022'][1][:12] == _lib.PROTOTYPES['salsa_nn.h']['salsa_nn_seld_score'][1][:12]
    src = open(os.path.join(ROOT, 'salsa_amd', 'csrc', 'seld_score.hip')).read()
    assert 'extern "C" int salsa_nn_seld_score2022(' in src and 'segment_sdi2022(' in src and 'class_record2022(' in src
    assert 'atomic' not in re.sub(r'//.*', '', src)                                        # fixed summation orders only
    assert '#include "../../salsa_amd/csrc/seld_score.h"' in open(os.path.join(ROOT, 'tests', 'hostemu', 'score2022_emu.cpp')).read()
    assert 'float ' not in re.sub(r'//.*', '', open(os.path.join(ROOT, 'salsa_amd', 'csrc', 'seld_score.h')).read())   # no float32 anywhere


@pytest.fixture(scope='module')
def lib():
    from salsa_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_launcher_refuses_what_the_2021_export_refuses_before_any_device_call(lib):
    """every call here returns E_INVAL from the host-side checks: nothing is launched, no pointer is read (they point nowhere).  The
    same bad argument is handed to salsa_nn_seld_score, which must refuse it too."""
    from salsa_amd import _lib
    outs22 = ('class_counters', 'class_de', 'sdi', 'status', 'file_counters', 'file_de', 'file_sdi')
    names = ('pred_rows', 'pred_counts', 'gt_rows', 'gt_counts') + outs22
    p = {k: C.c_void_p(0x1000 * (i + 1)) for i, k in enumerate(names)}
    good = dict(pred_capacity=7200, gt_capacity=900, n_files=4, n_frames=600, label_rate=10, n_classes=14, thr=20.0, margin=1e-4, **p)

    def call(**kw):
        a = dict(good, **kw)
        return lib.salsa_nn_seld_score2022(a['pred_rows'], a['pred_counts'], a['pred_capacity'], a['gt_rows'], a['gt_counts'], a['gt_capacity'],
                                           a['n_files'], a['n_frames'], a['label_rate'], a['n_classes'], a['thr'], a['margin'],
                                           *[a[k] for k in outs22], None)

    def call21(**kw):
        a = dict(good, **kw)
        return lib.salsa_nn_seld_score(a['pred_rows'], a['pred_counts'], a['pred_capacity'], a['gt_rows'], a['gt_counts'], a['gt_capacity'],
                                       a['n_files'], a['n_frames'], a['label_rate'], a['n_classes'], a['thr'], a['margin'], a['class_counters'],
                                       a['class_de'], a['status'], a['file_counters'], a['file_de'], None)
    for k in names[:8]:
        assert call(**{k: None}) == _lib.E_INVAL, k                                  # a NULL required pointer
    for k in outs22[4:]:
        assert call(**{k: None}) == _lib.E_INVAL, k                                  # the file sums come together or not at all
    for k in ('pred_rows', 'gt_rows', 'class_de', 'file_counters', 'file_de', 'file_sdi'):
        assert call(**{k: C.c_void_p(0x1004)}) == _lib.E_INVAL, k                    # 8-byte values
    for k, bad in (('n_classes', (0, -1, 33)), ('label_rate', (0, -10, 33)), ('n_files', (0, -2, 65536)), ('n_frames', (0, -600, 32768)),
                   ('pred_capacity', (0, -1)), ('gt_capacity', (0, -1)), ('margin', (-1e-9, float('nan'), float('inf'))),
                   ('thr', (float('nan'),))):
        for v in bad:
            assert call(**{k: v}) == call21(**{k: v}) == _lib.E_INVAL, (k, v)


# ---------------------------------------------------------------------------------------------------- host helpers of crnn/score.py
def test_merge_versions_and_the_consumers_know_2022():
    from salsa_amd.crnn import fit
    from salsa_amd.crnn.infer import infer_pipelined
    from salsa_amd.crnn.metrics import SeldMetrics2022
    from salsa_amd.crnn.score import (_VERSIONS, DEFAULT_MARGIN, DeviceSeldScore, DeviceSeldScore2020, DeviceSeldScore2022, resolve_records,
                                      score_dcase_rows)
    assert _VERSIONS['2022'] == (DeviceSeldScore2022, SeldMetrics2022, 'salsa_nn_seld_score2022') and sorted(_VERSIONS) == ['2020', '2021', '2022']
    a = DeviceSeldScore2022(n_classes=4)
    assert isinstance(a, SeldMetrics2022) and (a.label_rate, a.margin, a.average, a.n_segments, a.n_doubt, a.n_refused) == (10, DEFAULT_MARGIN, 'macro', 0, 0, 0)
    assert DeviceSeldScore2022(4, 20, 10, 1e-4, 'micro').average == 'micro'
    name, pred, gt, kw = cases22.main_case()
    parts = []
    for f in range(3):                                                                     # three sub-batches of one file, all "scored"
        m = cases22.host_total(pred[f:f + 1], gt[f:f + 1], kw)
        five = np.stack([getattr(m, n) for n in cases22.FIVE], axis=1)[None]
        parts.append(resolve_records(five, m.total_DE[None], np.zeros((1, 3), dtype=np.int32), None, eval_version='2022',
                                     sum_sdi=np.array([[m.S, m.D, m.I]]), **kw))
        assert a.merge(parts[-1]) is a
    assert a.n_segments == 9 and a.file_records()['TP'].shape == (3, 4)
    cases22.check_result(name, a, pred, gt, kw, 0.0)                                       # (the same host arithmetic: exact)
    for into, other in ((a, DeviceSeldScore(n_classes=4)), (DeviceSeldScore(n_classes=4), a), (DeviceSeldScore2020(n_classes=4), a),
                        (a, DeviceSeldScore2022(n_classes=5)), (a, SeldMetrics2022(4))):
        with pytest.raises(ValueError, match='merge'):
            into.merge(other)
    with pytest.raises(ValueError, match="decode='device'"):
        infer_pipelined(2, None, None, decode='host', score=(None, None, DeviceSeldScore2022()))
    with pytest.raises(ValueError, match='average'):
        DeviceSeldScore2022(average='weighted')
    for bad in ('2019', '2023'):
        with pytest.raises(ValueError, match='Unknown eval_version'):
            resolve_records(np.zeros(10), 0.0, np.zeros((1, 1)), None, eval_version=bad)
        with pytest.raises(ValueError, match='Unknown eval_version'):
            fit.validate(None, None, None, eval_version=bad)
        with pytest.raises(ValueError, match='Unknown eval_version'):
            score_dcase_rows(None, None, None, None, eval_version=bad)
