"""CPU tests of the device scorer's SELD 2020 statements (salsa_amd/csrc/seld_score.h built with g++: tests/hostemu/score2020_emu.cpp)
against crnn/metrics.py::SeldMetrics2020, of the 2020 side of crnn/score.py, of the export and of the launcher's argument checks.

What "bit-equal" is held against is what tests/test_seld_score_cpu.py's docstring says: the emulation calls the C library's sin / cos /
acos, numpy's arccos is not the C library's on every machine (at most 7.2e-13 degrees per distance), so total_DE is held BIT-EQUAL to
SeldMetrics2020 with only its `angular_distance_deg` routed through libm -- in every record in which no cell has a rival map within
`margin` of its best, for there the brute force and scipy add the same distances in the same order -- and within 4e-12 x DE_TP
degrees elsewhere and to the stock SeldMetrics2020 (a class average is a mean of sums of at most four distances).  The ten counters
are equal to the stock SeldMetrics2020's always.

Which segments go to the host.  Of the 505 segments of g12, the built families and the two knife-edge cases, 4 have a class average
within 1e-4 degrees of the threshold, all of them the built knife edges (files 0 and 1 of either case), and no cell of those inputs
holds more than 4 DOAs: no segment of g12 or of a built family may come back with status 1 or 2."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import seld_score_cases as cases
import seld_score2020_cases as cases20
from conftest import ROOT


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('score2020_emu') / 'libscore2020_emu.so')
    # -fno-builtin-sin / -cos: g++ otherwise merges sin(e) and cos(e) into one sincos call, whose results are not always sin's and cos's
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-fno-builtin-sin', '-fno-builtin-cos', '-o', so,
                           os.path.join(ROOT, 'tests', 'hostemu', 'score2020_emu.cpp')])
    L = C.CDLL(so)
    sp, ip, dp = C.POINTER(C.c_int16), C.POINTER(C.c_int), C.POINTER(C.c_double)
    L.emu_score2020_file.argtypes = [sp, C.c_int, sp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, ip, dp, ip]
    return L


@pytest.fixture(scope='module')
def LibmMetrics():
    """SeldMetrics2020 whose distances go through the C library's sin / cos / acos, statement for statement angular_distance_deg"""
    from salsa_amd.crnn import metrics

    def libm_distance(azi1, ele1, azi2, ele2):
        a1, e1, a2, e2 = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) * np.pi / 180. for v in (azi1, ele1, azi2, ele2)))
        out = np.empty(a1.shape)
        for i in np.ndindex(a1.shape):
            d = math.sin(e1[i]) * math.sin(e2[i]) + math.cos(e1[i]) * math.cos(e2[i]) * math.cos(abs(a1[i] - a2[i]))
            out[i] = math.acos(min(1.0, max(-1.0, d))) * 180 / np.pi
        return out

    class Libm(metrics.SeldMetrics2020):
        def update(self, *a, **kw):
            stock = metrics.angular_distance_deg
            metrics.angular_distance_deg = libm_distance
            try:
                super().update(*a, **kw)
            finally:
                metrics.angular_distance_deg = stock
    return Libm


def margin():
    from salsa_amd.crnn.score import DEFAULT_MARGIN
    return DEFAULT_MARGIN


def emu_records(emu, pred_files, gt_files, kw, margin):
    """-> counters (files, n_seg, 10), total_de (files, n_seg), status (files, n_seg) of the emulation, through score.pack_rows"""
    from salsa_amd.crnn.score import pack_rows
    (pr, pc), (gr, gc) = pack_rows(pred_files), pack_rows(gt_files)
    n_seg = -(-kw['n_frames'] // kw['label_rate'])
    counters = np.full((len(pred_files), n_seg, 10), -7, dtype=np.int32)
    de, status = np.full((len(pred_files), n_seg), np.nan), np.full((len(pred_files), n_seg), -7, dtype=np.int32)
    sp, ip, dp = C.POINTER(C.c_int16), C.POINTER(C.c_int), C.POINTER(C.c_double)
    for f in range(len(pred_files)):
        p, g = np.ascontiguousarray(pr[f]), np.ascontiguousarray(gr[f])
        emu.emu_score2020_file(p.ctypes.data_as(sp), int(pc[f]), g.ctypes.data_as(sp), int(gc[f]), kw['n_frames'], kw['label_rate'],
                               kw['n_classes'], float(kw['doa_threshold']), margin, counters[f].ctypes.data_as(ip), de[f].ctypes.data_as(dp),
                               status[f].ctypes.data_as(ip))
    return counters, de, status


def add_up(counters, de, status):
    """the scored records added up as the launch does: integers exactly, total_DE one running sum in record order"""
    ok = status.reshape(-1) == 0
    total = 0.0
    for v in de.reshape(-1)[ok]:
        total += float(v)
    return counters.reshape(-1, 10)[ok].astype(np.int64).sum(axis=0), total


def check_case(emu, LibmMetrics, name, pred_files, gt_files, kw, margin):
    """every record against SeldMetrics2020 on its segment alone, the status against numpy's own costs, and the totals after the host
    has scored the doubt / refused segments; returns the status array"""
    from salsa_amd.crnn.score import DeviceSeldScore2020, resolve_records
    counters, de, status = emu_records(emu, pred_files, gt_files, kw, margin)
    want_c, n_tied = np.zeros(10, dtype=np.int64), 0
    for f, (p, g) in enumerate(zip(pred_files, gt_files)):
        for s in range(status.shape[1]):
            what = '%s: file %d segment %d' % (name, f, s)
            assert status[f, s] == cases20.expected_status(p, g, s, kw, margin), what
            ref_c, ref_de = cases20.host_segment(p, g, s, kw)
            libm_c, libm_de = cases20.host_segment(p, g, s, kw, LibmMetrics)
            if status[f, s] == 0:
                assert list(counters[f, s]) == ref_c == libm_c, what
                if cases20.segment_clearance(p, g, s, kw)[0] > margin:
                    assert de[f, s] == libm_de, '%s: total_DE %r, SeldMetrics2020 over libm %r' % (what, de[f, s], libm_de)
                else:
                    n_tied += 1
                assert abs(de[f, s] - libm_de) <= cases20.NUMPY_ACOS_DEG4 * ref_c[cases20.DE_TP], what
                assert abs(de[f, s] - ref_de) <= cases20.NUMPY_ACOS_DEG4 * ref_c[cases20.DE_TP], what
            else:
                assert not counters[f, s].any() and de[f, s] == 0.0, what
            want_c += ref_c
    sums, sum_de = add_up(counters, de, status)
    got = resolve_records(sums, sum_de, status, lambda f: (pred_files[f], gt_files[f]), margin=margin, eval_version='2020', **kw)
    whole = cases20.host_total(pred_files, gt_files, kw)
    assert isinstance(got, DeviceSeldScore2020)
    assert [getattr(got, n) for n in cases20.COUNTERS] == [getattr(whole, n) for n in cases20.COUNTERS] == list(want_c), name
    assert abs(got.total_DE - whole.total_DE) <= cases20.NUMPY_ACOS_DEG4 * max(1, whole.DE_TP), name
    assert (got.n_segments, got.n_doubt, got.n_refused) == (status.size, int((status == 1).sum()), int((status == 2).sum()))
    if whole.Nref:
        assert got.scores() == pytest.approx(whole.scores(), rel=1e-12) and got.seld_error() == pytest.approx(whole.seld_error(), rel=1e-12)
    return status, n_tied


# ---------------------------------------------------------------------------------------------------- g12, built families, knife edges
def test_g12_as_one_batch_and_cumulatively(emu, LibmMetrics):
    from salsa_amd.crnn.metrics import SeldMetrics2020
    from salsa_amd.crnn.score import DeviceSeldScore2020, resolve_records
    pred, gt = cases.g12_files()
    status, _ = check_case(emu, LibmMetrics, 'g12', pred, gt, cases.DEFAULTS, margin())
    assert status.size == 240 and not status.any()                                         # nothing goes to the host
    acc, host = DeviceSeldScore2020(), SeldMetrics2020()
    for f in range(len(pred)):
        c, de, st = emu_records(emu, pred[f:f + 1], gt[f:f + 1], cases.DEFAULTS, margin())
        acc.merge(resolve_records(*add_up(c, de, st), st, lambda _: (pred[f], gt[f]), margin=margin(), eval_version='2020', **cases.DEFAULTS))
        host.update(pred[f], gt[f])
        assert [getattr(acc, n) for n in cases20.COUNTERS] == [getattr(host, n) for n in cases20.COUNTERS], f
        assert abs(acc.total_DE - host.total_DE) <= cases20.NUMPY_ACOS_DEG4 * host.DE_TP
        assert acc.scores() == pytest.approx(host.scores(), rel=1e-12)
    assert acc.n_segments == 240 and (acc.TP, acc.Nref, acc.Nsys, acc.DE_TP) == (113, 290, 219, 182)   # the reference's own (golden g29)


FAMILIES = cases.built_families()


@pytest.mark.parametrize('k', range(len(FAMILIES)), ids=[c[0].replace(' ', '_') for c in FAMILIES])
def test_built_family(emu, LibmMetrics, k):
    name, pred, gt, kw = FAMILIES[k]
    status, n_tied = check_case(emu, LibmMetrics, name, pred, gt, kw, margin())
    assert not status.any(), name                                                          # no doubt, nothing refused
    assert n_tied == 0, name                                                               # so every total_DE was held bit-equal
    whole = cases20.host_total(pred, gt, kw)
    if name == 'no common frame':
        c, _ = cases20.host_segment(pred[0], gt[0], 0, kw)                                 # class 3: both present, no common frame -> ONE miss
        assert [c[cases20.COUNTERS.index(n)] for n in ('FN', 'Nref', 'Nsys', 'DE_TP')] == [1, 1, 1, 0]
    elif name not in ('both empty', 'empty prediction', 'empty ground truth'):
        assert whole.DE_TP >= 10 and whole.FN > 0 and (whole.TP > 0 or 'cells' in name), name


def test_knife_edges_go_to_the_host_and_rival_maps_do_not(emu, LibmMetrics):
    """files 0 and 1 straddle the threshold (doubt); files 2 - 5 hold duplicate, equidistant and equal-cost pairings, which are doubt
    in the 2021 metric and none here: only the value of the minimum enters"""
    n_tied = 0
    for name, pred, gt, kw in cases.knife_edges():
        status, tied = check_case(emu, LibmMetrics, name, pred, gt, kw, margin())
        assert list(status[:, 0]) == [1, 1, 0, 0, 0, 0] and not status[:, 1].any(), name
        n_tied += tied
    assert n_tied == 8                                                                     # (and those totals were held within 4e-12 x DE_TP)
    from salsa_amd.crnn.metrics import SeldMetrics2020
    for thr, want in ((20, [1, 0]), (19.999999999999993, [1, 0]), (19.99999999999999, [0, 0]), (20.00000000000001, [1, 1])):
        got = []
        for a, b in (cases.KNIFE_BELOW, cases.KNIFE_ABOVE):
            m = SeldMetrics2020(12, thr)
            m.update([(0, 0) + b], [(0, 0) + a])
            got.append(m.TP)
        assert got == want, thr


def test_five_doas_in_a_cell_are_refused_and_scored_on_the_host(emu, LibmMetrics):
    name, files_p, files_g, kw = cases20.five_in_a_cell()
    status, _ = check_case(emu, LibmMetrics, name, files_p, files_g, kw, margin())
    assert list(status[:, 1]) == [2, 2, 0] and list(status[:, 2]) == [0, 0, 2] and not (status[:, [0, 3]] == 2).any() and not (status == 1).any()


# ---------------------------------------------------------------------------------------------------- the export and its checks
def test_seld_score2020_is_declared_listed_and_built_from_its_own_source():
    from salsa_amd import _lib
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'salsa_nn.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+salsa_nn_seld_score2020\s*\(', hdr) and 'salsa_nn_seld_score2020' in _lib.NN_EXPORTS
    assert _lib.PROTOTYPES['salsa_nn.h']['salsa_nn_seld_score2020'] == _lib.PROTOTYPES['salsa_nn.h']['salsa_nn_seld_score']
    assert os.path.join(ROOT, 'salsa_amd', 'csrc', 'seld_score.hip') in _lib.build_command()
    src = open(os.path.join(ROOT, 'salsa_amd', 'csrc', 'seld_score.hip')).read()
    assert 'extern "C" int salsa_nn_seld_score2020(' in src and '#include "seld_score.h"' in src
    assert '#include "../../salsa_amd/csrc/seld_score.h"' in open(os.path.join(ROOT, 'tests', 'hostemu', 'score2020_emu.cpp')).read()
    assert 'float ' not in re.sub(r'//.*', '', open(os.path.join(ROOT, 'salsa_amd', 'csrc', 'seld_score.h')).read())   # no float32 anywhere


@pytest.fixture(scope='module')
def lib():
    from salsa_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_launcher_refuses_invalid_arguments_before_any_device_call(lib):
    """every call here returns E_INVAL from the host-side checks: nothing is launched, no pointer is read (they point nowhere)"""
    from salsa_amd import _lib
    names = ('pred_rows', 'pred_counts', 'gt_rows', 'gt_counts', 'counters', 'total_de', 'status', 'sum_counters', 'sum_de')
    p = {k: C.c_void_p(0x1000 * (i + 1)) for i, k in enumerate(names)}
    good = dict(pred_capacity=7200, gt_capacity=900, n_files=4, n_frames=600, label_rate=10, n_classes=14, thr=20.0, margin=1e-4, **p)

    def call(**kw):
        a = dict(good, **kw)
        return lib.salsa_nn_seld_score2020(a['pred_rows'], a['pred_counts'], a['pred_capacity'], a['gt_rows'], a['gt_counts'], a['gt_capacity'],
                                           a['n_files'], a['n_frames'], a['label_rate'], a['n_classes'], a['thr'], a['margin'], a['counters'],
                                           a['total_de'], a['status'], a['sum_counters'], a['sum_de'], None)
    for k in names[:7]:
        assert call(**{k: None}) == _lib.E_INVAL, k                                  # a NULL required pointer
    assert call(sum_counters=None) == _lib.E_INVAL and call(sum_de=None) == _lib.E_INVAL    # the sums come together or not at all
    for k in ('pred_rows', 'gt_rows', 'total_de', 'sum_de', 'sum_counters'):
        assert call(**{k: C.c_void_p(0x1004)}) == _lib.E_INVAL, k                    # 8-byte values
    for k, bad in (('n_classes', (0, -1, 33)), ('label_rate', (0, -10, 33)), ('n_files', (0, -2, 65536)), ('n_frames', (0, -600, 32768)),
                   ('pred_capacity', (0, -1)), ('gt_capacity', (0, -1)), ('margin', (-1e-9, float('nan'), float('inf'))),
                   ('thr', (float('nan'),))):
        for v in bad:
            assert call(**{k: v}) == _lib.E_INVAL, (k, v)


# ---------------------------------------------------------------------------------------------------- host helpers of crnn/score.py
def test_merge_across_versions_raises_and_the_accumulator_needs_the_device_decoder():
    from salsa_amd.crnn.infer import infer_clips_sharded, infer_pipelined
    from salsa_amd.crnn.metrics import SeldMetrics2020
    from salsa_amd.crnn.score import DEFAULT_MARGIN, DeviceSeldScore, DeviceSeldScore2020, resolve_records
    assert DEFAULT_MARGIN == 1e-4 and DEFAULT_MARGIN >= 16 * 4 * 1.207e-6           # four distances of profiles/seld_score_distance.txt
    a, b = DeviceSeldScore2020(n_classes=14), DeviceSeldScore2020(n_classes=14)
    assert isinstance(a, SeldMetrics2020) and (a.label_rate, a.margin, a.n_segments, a.n_doubt, a.n_refused) == (10, DEFAULT_MARGIN, 0, 0, 0)
    b.TP, b.Nsys, b.TN, b.total_DE, b.n_doubt, b.n_segments = 3, 5, 7, 1.5, 2, 60
    assert a.merge(b) is a and (a.TP, a.Nsys, a.TN, a.total_DE, a.n_doubt, a.n_segments) == (3, 5, 7, 1.5, 2, 60)
    for into, other in ((a, DeviceSeldScore(n_classes=14)), (DeviceSeldScore(n_classes=14), a), (a, DeviceSeldScore2020(n_classes=12))):
        with pytest.raises(ValueError, match='merge'):
            into.merge(other)
    with pytest.raises(ValueError, match="decode='device'"):
        infer_pipelined(2, None, None, decode='host', score=(None, None, DeviceSeldScore2020()))
    with pytest.raises(ValueError, match="decode='device'"):
        infer_clips_sharded(['a', 'b'], None, None, score=(None, None, DeviceSeldScore2020()))
    with pytest.raises(ValueError, match='Unknown eval_version'):
        resolve_records(np.zeros(10), 0.0, np.zeros((1, 1)), None, eval_version='2019')
