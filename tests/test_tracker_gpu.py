"""The noise-floor tracker's gate mask (relayout_kernel -> tracker_kernel -> the covariance kernel's mask read), bit for bit,
on the built tracks of tests/tracker_reference.py.

    python -m pytest tests/test_tracker_gpu.py -q -m gpu -s

With cond_num = 0 the coherence test is vacuous, so `gate > 0` of SalsaExtractor.eigvec IS the tracker's indicator_sig.  It is
compared with the float64 restatement without tolerance and without excused bins, over chunk counts from 1 frame to 75 chunks
and a one-frame tail, one to seven 32-bin mask groups (odd group counts under the covariance kernel's two-group read), and batches
of 1, 3, 4 and 32 different clips.  test_tracker_cpu.py ties the restatement to the reference's masks and to the C oracle, and
shows that each case reaches its branch.  The largest case solves every gated bin of 32 x 200 x 4801 in float64.
Wall time of the file on one MI355X: 9 s (57 tests, 35.1 M mask bits compared, none differing), so the batch-32 case keeps its 200 bins."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import tracker_reference as tr

pytestmark = pytest.mark.gpu

CLOCK = {}


@pytest.fixture(scope='module', autouse=True)
def _clock():
    """started by this module's first test (collection of the other test files is not counted)"""
    CLOCK['t0'] = time.time()
    yield


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _extractor(**kw):
    from salsa_amd.extractor import SalsaExtractor
    kw.setdefault('cond_num', 0.0)
    kw.setdefault('fmax_doa', 9000 if kw.get('audio_format', 'foa') == 'foa' else 4000)
    return SalsaExtractor(**kw)


def _gate(ex, Xd):
    _, gate = ex.eigvec(Xd, lower_bin=1, return_gate=True)
    return gate


@pytest.mark.parametrize('name', tr.CASE_NAMES)
def test_gate_mask_is_the_restatement_bit_for_bit(dev, name):
    X, _ = tr.build_case(name)
    B = X.shape[0]
    want = tr.tracker_mask(X)
    Xd = torch.from_numpy(X).to(dev)
    ex = _extractor()
    gate = _gate(ex, Xd)
    g = gate.cpu().numpy()
    assert g.max() <= 2
    got = g > 0
    print('%-20s %s density %.4f, %d bits compared, %d differ' % (name, X.shape[:3], want.mean(), want.size, int((got != want).sum())))
    assert np.array_equal(got, want), tr.describe_first_difference(got, want, X)
    assert torch.equal(_gate(ex, Xd), gate), 'two runs differ'
    if B > 1:                                                # clip indexing: each clip alone, and the batch reversed
        for b in range(B):
            assert torch.equal(_gate(ex, Xd[b:b + 1].contiguous())[0], gate[b]), 'clip %d alone differs from the batch' % b
        assert torch.equal(_gate(ex, Xd.flip(0).contiguous()).flip(0), gate), 'the reversed batch differs'
    if name in tr.FORMAT_SUBSET:                             # the tracker sees channel 0 only
        assert torch.equal(_gate(_extractor(audio_format='mic'), Xd) > 0, gate > 0), 'FOA and MIC masks differ'


# (the batch-32 block is left out: its shape is the batch-4 block's, and a second 1 GB block and float64 output buy nothing here)
@pytest.mark.parametrize('name', [n for n in tr.CASE_NAMES if (tr.case(n)[4] % tr.TR_CH or tr.case(n)[3] % tr.TR_BINS) and tr.case(n)[2] <= 4])
def test_ragged_shapes_leave_no_gate_byte_unwritten(dev, name):
    """SalsaExtractor.eigvec hands the library torch.empty buffers; here the gate starts at 255 (the kernel writes 0 / 1 / 2 only)
    and the output at NaN, through the C ABI directly."""
    from salsa_amd import _lib
    L = _lib.load()
    X, _ = tr.build_case(name)
    B, nb, nt, _ = X.shape
    Xd = torch.from_numpy(X).to(dev)
    ex = _extractor()
    out_m, gate_m = ex.eigvec(Xd, lower_bin=1, return_gate=True)
    out = torch.full((B, 3, nb, nt), float('nan'), dtype=torch.float64, device=dev)
    gate = torch.full((B, nb, nt), 255, dtype=torch.uint8, device=dev)
    ws = torch.empty(int(L.salsa_eigvec_workspace_bytes(ex._plan, B, nb, nt)) + 256, dtype=torch.uint8, device=dev)
    rc = L.salsa_eigvec_batch(ex._plan, C.c_void_p(Xd.data_ptr()), B, nb, nt, 1, C.c_void_p(out.data_ptr()),
                              C.c_void_p(gate.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(),
                              C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0
    torch.cuda.synchronize(dev)
    assert int((gate == 255).sum()) == 0, '%d gate bytes were never written' % int((gate == 255).sum())
    assert torch.equal(gate, gate_m)
    assert np.array_equal(gate.cpu().numpy() > 0, tr.tracker_mask(X))
    assert not torch.isnan(out).any() and torch.equal(out, out_m)


@pytest.mark.parametrize('name', tr.SOLVER_SUBSET)
def test_production_solver_reads_the_same_mask(dev, name):
    """cond_num 5 through salsa_eigvec_feature_batch (the packed-float32 instantiation extract() launches): its counter of gated
    frames is the number of set mask bits."""
    X, _ = tr.build_case(name)
    want = tr.tracker_mask(X)
    Xd = torch.from_numpy(X).to(dev)
    for fmt in ('foa', 'mic'):
        ex = _extractor(audio_format=fmt, cond_num=5.0)
        ex.set_stats(True)
        ex.eigvec_features(Xd, 1)
        st = ex.read_stats()
        assert st['gated_frames'] == int(want.sum()), (name, fmt, st, int(want.sum()))


def test_zz_report_time():
    print('tracker GPU tests: %.1f s' % (time.time() - CLOCK['t0']))
