"""CPU tests of the device SELD scorer's statements (salsa_amd/csrc/seld_score.h built with g++: tests/hostemu/score_emu.cpp) against
crnn/metrics.py::SeldMetrics, of the host half of crnn/score.py, of the export and of the launcher's argument checks.

What "bit-equal" is held against.  The emulation calls the C library's sin / cos / acos.  numpy's float64 arccos is NOT the C library's on
every machine: where numpy dispatches to its AVX-512 loops, 9 % of arccos results differ from libm's by one ulp (measured: 9311 of
100001 arguments in [-1, 1]; sin and cos agree on every integer degree), so `angular_distance_deg` differs from the emulation's distance
in 8 % of direction pairs, by at most 7.2e-13 degrees.  total_DE is therefore held BIT-EQUAL to `SeldMetrics` with only its
`angular_distance_deg` routed through libm (LibmMetrics below: the same update, the same scipy, the same summation order), and to
the stock `SeldMetrics` within DE_TP x 1e-12 degrees (each average within the 7.2e-13 above); the ten counters are equal to the
stock SeldMetrics' always.  Totals over several records are one running float64 sum in record order (what the device adds up),
then the host-scored segments in record order."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import seld_score_cases as cases
from conftest import ROOT

NUMPY_ACOS_DEG = 1e-12                                   # see the module docstring


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('score_emu') / 'libscore_emu.so')
    # -fno-builtin-sin / -cos: g++ otherwise merges sin(e) and cos(e) into one sincos call, whose results are not always sin's and cos's
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-fno-builtin-sin', '-fno-builtin-cos', '-o', so,
                           os.path.join(ROOT, 'tests', 'hostemu', 'score_emu.cpp')])
    L = C.CDLL(so)
    sp, ip, dp = C.POINTER(C.c_int16), C.POINTER(C.c_int), C.POINTER(C.c_double)
    L.emu_distance.restype = C.c_double
    L.emu_distance.argtypes = [C.c_int] * 4
    L.emu_n_segments.argtypes = [C.c_int, C.c_int]
    L.emu_score_file.argtypes = [sp, C.c_int, sp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, ip, dp, ip]
    return L


@pytest.fixture(scope='module')
def LibmMetrics():
    """SeldMetrics whose distances go through the C library's sin / cos / acos, statement for statement angular_distance_deg"""
    from salsa_amd.crnn import metrics

    def libm_distance(azi1, ele1, azi2, ele2):
        a1, e1, a2, e2 = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) * np.pi / 180. for v in (azi1, ele1, azi2, ele2)))
        out = np.empty(a1.shape)
        for i in np.ndindex(a1.shape):
            d = math.sin(e1[i]) * math.sin(e2[i]) + math.cos(e1[i]) * math.cos(e2[i]) * math.cos(abs(a1[i] - a2[i]))
            out[i] = math.acos(min(1.0, max(-1.0, d))) * 180 / np.pi
        return out

    class Libm(metrics.SeldMetrics):
        def update(self, *a, **kw):
            stock = metrics.angular_distance_deg
            metrics.angular_distance_deg = libm_distance
            try:
                super().update(*a, **kw)
            finally:
                metrics.angular_distance_deg = stock
    return Libm


def emu_records(emu, pred_files, gt_files, kw, margin):
    """-> counters (files, n_seg, 10), total_de (files, n_seg), status (files, n_seg) of the emulation, through score.pack_rows"""
    from salsa_amd.crnn.score import pack_rows
    (pr, pc), (gr, gc) = pack_rows(pred_files), pack_rows(gt_files)
    n_seg = emu.emu_n_segments(kw['n_frames'], kw['label_rate'])
    assert n_seg == int(np.ceil(kw['n_frames'] / float(kw['label_rate'])))
    counters = np.full((len(pred_files), n_seg, 10), -7, dtype=np.int32)
    de, status = np.full((len(pred_files), n_seg), np.nan), np.full((len(pred_files), n_seg), -7, dtype=np.int32)
    sp, ip, dp = C.POINTER(C.c_int16), C.POINTER(C.c_int), C.POINTER(C.c_double)
    for f in range(len(pred_files)):
        p, g = np.ascontiguousarray(pr[f]), np.ascontiguousarray(gr[f])
        emu.emu_score_file(p.ctypes.data_as(sp), int(pc[f]), g.ctypes.data_as(sp), int(gc[f]), kw['n_frames'], kw['label_rate'],
                           kw['n_classes'], float(kw['doa_threshold']), margin, counters[f].ctypes.data_as(ip), de[f].ctypes.data_as(dp),
                           status[f].ctypes.data_as(ip))
    return counters, de, status


def add_up(counters, de, status):
    """the scored records added up as salsa_nn_seld_score does: integers exactly, total_DE one running sum in record order"""
    ok = status.reshape(-1) == 0
    total = 0.0
    for v in de.reshape(-1)[ok]:
        total += float(v)
    return counters.reshape(-1, 10)[ok].astype(np.int64).sum(axis=0), total


def check_case(emu, LibmMetrics, name, pred_files, gt_files, kw, margin):
    """every record against SeldMetrics on its segment alone, the status sets against numpy's own costs, and the totals after the
    host has scored the doubt / refused segments; returns the status array"""
    from salsa_amd.crnn.score import resolve_records
    counters, de, status = emu_records(emu, pred_files, gt_files, kw, margin)
    want_c, want_de = np.zeros(10, dtype=np.int64), 0.0
    late = []
    for f, (p, g) in enumerate(zip(pred_files, gt_files)):
        for s in range(status.shape[1]):
            what = '%s: file %d segment %d' % (name, f, s)
            assert status[f, s] == cases.expected_status(p, g, s, kw, margin), what
            ref_c, ref_de = cases.host_segment(p, g, s, kw)
            libm_c, libm_de = cases.host_segment(p, g, s, kw, LibmMetrics)
            if status[f, s] == 0:
                assert list(counters[f, s]) == ref_c == libm_c, what
                assert de[f, s] == libm_de, '%s: total_DE %r, SeldMetrics over libm %r' % (what, de[f, s], libm_de)
                assert abs(de[f, s] - ref_de) <= NUMPY_ACOS_DEG * ref_c[7], what
                want_de += libm_de
            else:
                assert not counters[f, s].any() and de[f, s] == 0.0, what
                late.append(ref_de)
            want_c += ref_c
    for v in late:
        want_de += v
    sums, sum_de = add_up(counters, de, status)
    got = resolve_records(sums, sum_de, status, lambda f: (pred_files[f], gt_files[f]), margin=margin, **kw)
    assert [getattr(got, n) for n in cases.COUNTERS] == list(want_c), name
    whole = cases.host_total(pred_files, gt_files, kw)
    assert [getattr(got, n) for n in cases.COUNTERS] == [getattr(whole, n) for n in cases.COUNTERS], name
    # the device's running sum over libm's distances, then the host's own segments (stock SeldMetrics): the same additions
    assert got.total_DE == want_de, '%s: total_DE %r, expected %r' % (name, got.total_DE, want_de)
    assert abs(got.total_DE - whole.total_DE) <= NUMPY_ACOS_DEG * max(1, whole.DE_TP), name
    assert (got.n_segments, got.n_doubt, got.n_refused) == (status.size, int((status == 1).sum()), int((status == 2).sum()))
    assert got.scores() == pytest.approx(whole.scores(), rel=1e-12) and got.seld_error() == pytest.approx(whole.seld_error(), rel=1e-12)
    return status


def margin():
    from salsa_amd.crnn.score import DEFAULT_MARGIN
    return DEFAULT_MARGIN


# ---------------------------------------------------------------------------------------------------- the distance statement
def test_distance_statement_is_the_hosts(emu):
    from salsa_amd.crnn.metrics import angular_distance_deg
    assert emu.emu_distance(0, 0, 20, 0) == 19.999999999999993 == float(angular_distance_deg(0, 0, 20, 0))
    assert emu.emu_distance(10, -10, 10, 10) == 20.00000000000001 == float(angular_distance_deg(10, -10, 10, 10))
    rng = np.random.RandomState(0)
    q = np.stack([rng.randint(-180, 180, 4000), rng.randint(-90, 91, 4000), rng.randint(-180, 180, 4000), rng.randint(-90, 91, 4000)], axis=1)
    q[:8] = [(0, 0, 0, 0), (0, 90, 77, 90), (0, -90, 0, 90), (-180, 0, 180, 0), (179, 0, -180, 0), (5, 5, 5, 5), (0, 0, 180, 0), (30, 89, 31, 89)]
    got = np.array([emu.emu_distance(*map(int, r)) for r in q])
    pi = np.pi
    want = []
    for a1, e1, a2, e2 in q.astype(np.float64) * pi / 180.:
        d = math.sin(e1) * math.sin(e2) + math.cos(e1) * math.cos(e2) * math.cos(abs(a1 - a2))
        want.append(math.acos(min(1.0, max(-1.0, d))) * 180 / pi)
    assert np.array_equal(got, np.array(want))                                       # the statement order, no fma: libm for libm
    ref = angular_distance_deg(q[:, 0], q[:, 1], q[:, 2], q[:, 3])
    print('distance: %d of %d differ from numpy, by at most %.3g degrees' % ((got != ref).sum(), len(q), np.abs(got - ref).max()))
    assert np.abs(got - ref).max() <= NUMPY_ACOS_DEG                                 # numpy's own arccos: the docstring's bound


# ---------------------------------------------------------------------------------------------------- g12
def test_g12_as_one_batch_and_cumulatively(emu, LibmMetrics):
    from salsa_amd.crnn.metrics import SeldMetrics
    from salsa_amd.crnn.score import DeviceSeldScore, resolve_records
    pred, gt = cases.g12_files()
    assert max(len(v) for rows in pred + gt for v in _cells(rows).values()) == 2          # up to 2 DOAs per cell on both sides
    status = check_case(emu, LibmMetrics, 'g12', pred, gt, cases.DEFAULTS, margin())
    share = float((status == 0).mean())
    print('g12: %d segments, %d in doubt, %d refused' % (status.size, (status == 1).sum(), (status == 2).sum()))
    assert share >= 0.5 and not (status == 2).any()
    # cumulatively: one file at a time merged into an accumulator, against SeldMetrics after each file
    acc, host = DeviceSeldScore(), SeldMetrics()
    for f in range(len(pred)):
        c, de, st = emu_records(emu, pred[f:f + 1], gt[f:f + 1], cases.DEFAULTS, margin())
        acc.merge(resolve_records(*add_up(c, de, st), st, lambda _: (pred[f], gt[f]), margin=margin(), **cases.DEFAULTS))
        host.update(pred[f], gt[f])
        assert [getattr(acc, n) for n in cases.COUNTERS] == [getattr(host, n) for n in cases.COUNTERS], f
        assert abs(acc.total_DE - host.total_DE) <= NUMPY_ACOS_DEG * host.DE_TP
        assert acc.scores() == pytest.approx(host.scores(), rel=1e-12)
    assert acc.n_segments == 240


def _cells(rows):
    out = {}
    for r in rows:
        out.setdefault((r[0], r[1]), []).append(r[2:])
    return out


# ---------------------------------------------------------------------------------------------------- built families, knife edges
FAMILIES = cases.built_families()


@pytest.mark.parametrize('k', range(len(FAMILIES)), ids=[c[0].replace(' ', '_') for c in FAMILIES])
def test_built_family(emu, LibmMetrics, k):
    name, pred, gt, kw = FAMILIES[k]
    status = check_case(emu, LibmMetrics, name, pred, gt, kw, margin())
    assert (status == 0).mean() >= 0.5 and not (status == 2).any(), name
    whole = cases.host_total(pred, gt, kw)
    if name == 'no common frame':
        c, _ = cases.host_segment(pred[0], gt[0], 0, kw)
        assert c[cases.COUNTERS.index('FN')] == 2 and c[cases.COUNTERS.index('DE_FN')] == 2 and c[cases.COUNTERS.index('Nref')] == 1
    elif name not in ('both empty', 'empty prediction', 'empty ground truth'):
        assert whole.DE_TP > 10 and whole.TP > 0 and whole.FP > 0, name                     # hits and misses both occur


def test_knife_edges_go_to_the_host(emu, LibmMetrics):
    for name, pred, gt, kw in cases.knife_edges():
        status = check_case(emu, LibmMetrics, name, pred, gt, kw, margin())
        assert list(status[:, 0]) == [1] * len(pred) and list(status[:, 1]) == [0] * len(pred), name
    # the two pairs really straddle: the host counts one as a hit and one as a miss at 20, and both as they fall at the other edge
    from salsa_amd.crnn.metrics import SeldMetrics
    for thr, want in ((20, [1, 0]), (19.999999999999993, [1, 0]), (19.99999999999999, [0, 0]), (20.00000000000001, [1, 1])):
        got = []
        for a, b in (cases.KNIFE_BELOW, cases.KNIFE_ABOVE):
            m = SeldMetrics(12, thr)
            m.update([(0, 0) + b], [(0, 0) + a])
            got.append(m.TP)
        assert got == want, thr


def test_five_doas_in_a_cell_are_refused_and_scored_on_the_host(emu, LibmMetrics):
    rng = np.random.RandomState(5)
    pred, gt = cases.random_file(rng, max_g=2, max_p=2, density=0.3)
    five = [(13, 6, 20 * k, 5) for k in range(5)]
    files_p, files_g = [pred + five, pred, pred + [(25, 0, 0, 0)] * 7], [gt + [(13, 6, 3, 3)], gt + five, gt]
    status = check_case(emu, LibmMetrics, 'five in a cell', files_p, files_g, dict(cases.DEFAULTS, n_frames=40), margin())
    assert list(status[:, 1]) == [2, 2, 0] and list(status[:, 2]) == [0, 0, 2] and not (status[:, [0, 3]] == 2).any()


# ---------------------------------------------------------------------------------------------------- the export and its checks
def test_seld_score_is_declared_listed_and_built_from_its_own_source():
    from salsa_amd import _lib
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'salsa_nn.h')).read(), flags=re.S)
    for name in ('salsa_nn_seld_score', 'salsa_nn_seld_distance'):
        assert re.search(r'\bint\s+%s\s*\(' % name, hdr) and name in _lib.NN_EXPORTS
    assert os.path.join(ROOT, 'salsa_amd', 'csrc', 'seld_score.hip') in _lib.build_command()
    src = open(os.path.join(ROOT, 'salsa_amd', 'csrc', 'seld_score.hip')).read()
    assert '#include "seld_score.h"' in src and '#include "build_guard.h"' in src
    assert '#include "../../salsa_amd/csrc/seld_score.h"' in open(os.path.join(ROOT, 'tests', 'hostemu', 'score_emu.cpp')).read()
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
    good = dict(pred_capacity=7200, gt_capacity=900, n_files=4, n_frames=600, label_rate=10, n_classes=12, thr=20.0, margin=1e-4, **p)

    def call(**kw):
        a = dict(good, **kw)
        return lib.salsa_nn_seld_score(a['pred_rows'], a['pred_counts'], a['pred_capacity'], a['gt_rows'], a['gt_counts'], a['gt_capacity'],
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
    assert lib.salsa_nn_seld_distance(None, 4, p['total_de'], None) == _lib.E_INVAL
    assert lib.salsa_nn_seld_distance(p['pred_rows'], 0, p['total_de'], None) == _lib.E_INVAL


# ---------------------------------------------------------------------------------------------------- host helpers of crnn/score.py
def test_gt_rows_to_device_packs_and_refuses():
    import torch
    from salsa_amd.crnn.metrics import load_dcase_csv  # noqa: F401  (5-column rows are its (frame, class, azimuth, elevation, track))
    from salsa_amd.crnn.score import gt_rows_to_device, pack_rows
    rows, counts = gt_rows_to_device([[(3, 1, -170, 45)], [], [(0, 0, 10.0, -5.0, 2), (599, 11, -180, 90, 0)]], torch.device('cpu'))
    assert rows.dtype == torch.int16 and counts.dtype == torch.int32 and rows.shape == (3, 2, 4) and counts.tolist() == [1, 0, 2]
    assert rows[0, 0].tolist() == [3, 1, -170, 45] and rows[2].tolist() == [[0, 0, 10, -5], [599, 11, -180, 90]] and not rows[1].any()
    assert pack_rows([[], []])[0].shape == (2, 1, 4)
    for bad in ([[(0, 0, 10.5, 0)]], [[(0, 0, 40000, 0)]], [[(-40000, 0, 0, 0)]], [[(0, 0, 0)]], [[(0, 0, 0, 0, 0, 0)]],
                [[(0, 0, float('nan'), 0)]], [[(0, 0, 1, 1), (0, 0, 1)]], [[(0.5, 0, 1, 1)]], []):
        with pytest.raises(ValueError):
            gt_rows_to_device(bad, torch.device('cpu'))


def test_score_keyword_needs_the_device_decoder():
    from salsa_amd.crnn.infer import infer_clips_sharded, infer_pipelined
    from salsa_amd.crnn.score import DeviceSeldScore
    with pytest.raises(ValueError, match="decode='device'"):
        infer_pipelined(2, None, None, decode='host', score=(None, None, DeviceSeldScore()))
    with pytest.raises(ValueError, match="decode='device'"):
        infer_clips_sharded(['a', 'b'], None, None, score=(None, None, DeviceSeldScore()))
    a, b = DeviceSeldScore(), DeviceSeldScore()
    b.TP, b.total_DE, b.n_doubt, b.n_segments = 3, 1.5, 2, 60
    assert a.merge(b) is a and (a.TP, a.total_DE, a.n_doubt, a.n_segments) == (3, 1.5, 2, 60)
    with pytest.raises(ValueError):
        a.merge(DeviceSeldScore(n_classes=14))
