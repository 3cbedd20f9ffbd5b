"""The DOA histogram kernel off its default shapes: the edge cases of tests/test_doa_hist_edges_cpu.py, each
through everything tests/test_doa_hist_gpu.py checks of a built case (check_kernel_case: guard bands, every element written, decisions
exact under the reference's margin condition, scores, spectrum and directions within the reference's derived bounds, the spectrum at a
peak equal to its score bit for bit, equal bits on two runs, with and without the spectrum and for a clip alone, the public call, the
torch path on the device, torch against the kernel); exact ties on the kernel and on the torch path on the device; and localize on a side
stream.  The grid step names the kernel's instantiation: doa_hist_kernel<4> up to 1024 cells (steps 15, 18, 30; 10 with 614 cells
too), <10> up to 2560 (steps 5, 6, 9), <28> beyond (step 3, 7082 cells); each test prints the one it reached.

MEASURED_EDGES below: the largest (error) / (bound) ratios, group by group.  Records of one run, not thresholds."""
import numpy as np
import pytest
import torch

from salsa_amd import localize as lz
from test_attn_gpu import DEV
from test_doa_hist_cpu import as_dict, built
from test_doa_hist_edges_cpu import EDGE_CASES, EDGE_IDS, TIE_BUILDERS, TIE_IDS, built_edge, check_ties
from test_doa_hist_gpu import _bits_equal, _run_guarded, check_kernel_case

pytestmark = pytest.mark.gpu
MEASURED_EDGES = """largest ratio (error) / (bound of tests/doa_hist_reference.py) over the cases and built frames of each group, both formats, on
one MI355X (profiles/doa_hist_edges_pytest_gpu.log); decisions (count, cell, n_votes) were equal to the reference's in every frame,
and no defect was found in the kernel, the torch path or the bounds:
                                           salsa_doa_hist               torch on device              torch against the kernel
                                           score  direction  spectrum   score  direction  spectrum   score  direction  spectrum
  (a) steps 3, 6, 9, 10, 18, 30            0.13   0.11       0.33       0.16   0.10       0.39       0.14   0.10       0.33
  (b) windows, (c) 63 / 64 / 65 votes      0.06   0.07       0.42       0.06   0.09       0.41       0.04   0.15       0.48
  (d) K = 8, eight and nine clusters       0.06   0.07       0.36       0.05   0.07       0.36       0.06   0.05       0.49
  (e) thresholds off their defaults        0.07   0.09       0.30       0.07   0.09       0.30       0.06   0.06       0.33
  (f) lengths float32 cannot square        0.03   0.04       0.20       0.02   0.04       0.20       0.03   0.03       0.32
The 4096-vote window at step 3, the largest case: score 0.06, direction 0.02, spectrum 0.27 of the bounds; 0.25 s."""


def _instantiation(loc):
    return 4 if loc.n_cells <= 4 * 256 else 10 if loc.n_cells <= 10 * 256 else 28


@pytest.mark.parametrize('name', EDGE_IDS)
def test_kernel_on_the_edge_cases(name, monkeypatch):
    loc, xs, refs = built_edge(name)
    c = EDGE_CASES[name]
    print('INSTANTIATION %s %s step %d: %d cells, doa_hist_kernel<%d>, window [%d, %d) x %d, K = %d'
          % (name, c['fmt'], c['step'], loc.n_cells, _instantiation(loc), loc.col0, loc.col1, loc.frames_per_label, loc.max_sources))
    worst = check_kernel_case(loc, xs, refs, name, monkeypatch)
    for leg, ratios in sorted(worst.items()):
        print('EDGE-RATIOS %s %s %s %s' % (c['group'], c['fmt'], leg, ' '.join('%s %.3f' % kv for kv in sorted(ratios.items()))))


@pytest.mark.parametrize('builder,step', TIE_BUILDERS, ids=TIE_IDS)
def test_exact_ties_go_to_the_lowest_index(builder, step, monkeypatch):
    """the frames of the CPU test (which proves that their scores tie bit for bit and says which waves the tied cells fall in) on the
    kernel -- the per-thread scan, the wave butterfly and the merge of the waves' winners -- and on the torch path on the device"""
    loc, x_host, expect = builder(step)
    x = torch.from_numpy(x_host.copy()).to(DEV)
    print('INSTANTIATION %s foa step %d: %d cells, doa_hist_kernel<%d>' % (builder.__wrapped__.__name__, step, loc.n_cells, _instantiation(loc)))
    res = _run_guarded(loc, x)
    check_ties(as_dict(res), expect, 'hip')
    assert _bits_equal(_run_guarded(loc, x, spectrum=False), res)
    monkeypatch.setattr(lz, 'HIP_DOA', False)
    torch_res = loc.localize(x, spectrum=True)
    monkeypatch.setattr(lz, 'HIP_DOA', True)
    assert torch_res.count.is_cuda
    check_ties(as_dict(torch_res), expect, 'torch on device')
    for f in ('count', 'n_votes', 'cell') + (('score',) if expect[0][2] is not None else ()):      # on the axes nothing rounds: the two
        assert torch.equal(getattr(torch_res, f), getattr(res, f)), f                              # legs' scores agree to the bit


def test_localize_on_a_side_stream_gives_the_same_bits():
    loc, xs, _ = built('foa', 7, 2, 5)
    x = torch.from_numpy(xs[0].copy()).to(DEV)
    base = loc.localize(x, spectrum=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream(DEV) == side
        other = loc.localize(x, spectrum=True)
    side.synchronize()
    assert _bits_equal(other, base)
