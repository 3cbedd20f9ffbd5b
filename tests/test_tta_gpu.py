"""GPU tests of test-time augmentation and ensembling: salsa_nn_tta_variant against the torch swaps and
salsa_nn_tta_merge against the restatement of tests/tta_reference.py, bit for bit; TtaForward and infer_pipelined(tta=) around a real
Trainer whose inputs and outputs are recorded (so nothing depends on the forward repeating itself); and SALSA_HIP_TTA=0 in a fresh
process against the HIP path."""
import os
import subprocess
import sys

import pytest
import torch

import tta_reference as ref
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---------------------------------------------------------------------------------------------------- 1. the variant kernel
def _views(kind, B, T, F, seed):
    """the shapes salsa_nn_tta_variant meets: dense, time-cropped, batch-strided, and a dense tensor 4 bytes off a 16-byte line"""
    Cn = ref.CHANNELS[kind]
    g = torch.Generator().manual_seed(seed)
    full = torch.randn(2 * B, Cn, T, F, generator=g).to(DEV)
    flat = torch.randn(B * Cn * T * F + 1, generator=g).to(DEV)
    return {'dense': full[:B], 'time-cropped': full[:B, :, 2:T - 1], 'batch-strided': full[::2], 'offset': flat[1:].view(B, Cn, T, F)}


@pytest.mark.parametrize('kind,B,T,F', [('foa', 3, 11, 200), ('mic', 3, 11, 200), ('gcc', 3, 11, 128), ('gcc', 2, 6, 25), ('mic', 2, 6, 25)])
def test_tta_variant_kernel_equals_the_torch_swaps(kind, B, T, F):
    from salsa_amd.crnn.tta import tta_variant
    for name, x in _views(kind, B, T, F, seed=T * F).items():
        assert (name != 'offset' or x.data_ptr() % 16 == 4) and (name in ('dense', 'offset')) == x.is_contiguous()
        keep = x.clone()
        out = torch.full(x.shape, float('nan'), device=DEV)
        assert tta_variant(x, kind, 0) is x
        for v in range(1, ref.V[kind]):
            out.fill_(float('nan'))
            got = tta_variant(x, kind, v, out=out)
            assert got.data_ptr() == out.data_ptr()                                          # the kernel wrote it: no torch path
            assert same_bits(got, ref.variant(x, kind, v)), (name, v)
        assert same_bits(x, keep), name                                                        # the input is only read
        assert not same_bits(tta_variant(x, kind, 1), x)


# ---------------------------------------------------------------------------------------------------- 2. the merge kernel
@pytest.mark.parametrize('nc', [12, 14])
def test_tta_merge_kernel_equals_the_restatement(nc):
    from salsa_amd.crnn import tta
    assert tta.USE_HIP_TTA
    for kind, n_models, ids in ref.MERGE_CASES:
        prob, xyz = ref.slab_case(kind, nc, n_models, ids)
        want_p, want_d = ref.merge(list(prob), list(xyz), n_models, ids, kind, nc)
        got_p, got_d = tta.tta_merge(prob.to(DEV), xyz.to(DEV), n_models, ids, kind, nc)
        assert got_p.is_cuda and same_bits(got_p, want_p) and same_bits(got_d, want_d), (kind, n_models, ids)


# ---------------------------------------------------------------------------------------------------- 3. TtaForward on a Trainer
def _slab_order(outputs, n_models, nv):
    return [outputs[vi * n_models + mi] for mi in range(n_models) for vi in range(nv)]


@pytest.fixture(scope='module')
def features():
    return torch.randn(3, 7, 160, 200, generator=torch.Generator().manual_seed(21)).to(DEV)


@pytest.fixture(scope='module')
def trainer():
    from salsa_amd.crnn.train import Trainer
    torch.manual_seed(0)
    return Trainer(DEV, total_steps=10 ** 6)


def test_ttaforward_around_a_recording_trainer(trainer, features):
    from salsa_amd.crnn.tta import TtaForward
    ins, outs = [], []
    tf = TtaForward(ref.recording(trainer.infer, ins, outs), 'foa', 'salsa')
    p, d = tf(features)
    assert len(ins) == 16 and p.shape == (3, 20, 12) and d.shape == (3, 20, 36) and p.dtype == d.dtype == torch.float32
    for v, xin in enumerate(ins):
        assert same_bits(xin, ref.variant(features, 'foa', v)), v
    want_p, want_d = ref.merge([o[0].cpu() for o in outs], [o[1].cpu() for o in outs], 1, list(range(16)), 'foa', 12)
    assert same_bits(p, want_p) and same_bits(d, want_d)
    # two models and a subset in list order, on the kept buffers of a second call
    ins.clear(), outs.clear()
    two = TtaForward([ref.recording(trainer.infer, ins, outs), ref.recording(ref.indexing_forward(), ins, outs)], 'foa', 'salsa',
                     variants=[5, 0, 9])
    for x in (features, features[:2]):
        ins.clear(), outs.clear()
        p, d = two(x)
        rec = _slab_order(outs, 2, 3)
        want_p, want_d = ref.merge([o[0].cpu() for o in rec], [o[1].cpu() for o in rec], 2, [5, 0, 9], 'foa', 12)
        assert len(outs) == 6 and same_bits(p, want_p) and same_bits(d, want_d)


def test_trainer_infer_tta_with_accdoa_takes_the_length_of_the_merged_vectors(features):
    from salsa_amd.crnn.nn_ops import accdoa_sed
    from salsa_amd.crnn.train import Trainer
    torch.manual_seed(1)
    tr = Trainer(DEV, total_steps=10 ** 6, output_format='accdoa')
    ins, outs = [], []
    plain_infer = tr.infer
    tr.infer = ref.recording(plain_infer, ins, outs)                                           # (infer_tta wraps self.infer)
    p, d = tr.infer_tta(features, 'foa')
    assert len(outs) == 16
    want_p, want_d = ref.merge([o[0].cpu() for o in outs], [o[1].cpu() for o in outs], 1, list(range(16)), 'foa', 12)
    assert same_bits(d, want_d) and same_bits(p, accdoa_sed(d, 12)) and not same_bits(p, want_p)
    assert tr.infer_tta(features, 'foa', variants=[3])[0].shape == (3, 20, 12) and len(tr._tta) == 2


# ---------------------------------------------------------------------------------------------------- 4. infer_pipelined(tta=)
@pytest.mark.parametrize('decode', ['device', 'host'])
@pytest.mark.parametrize('chunked', [False, True])
def test_infer_pipelined_with_tta_decodes_the_restated_merge(trainer, features, chunked, decode):
    """MIC TTA (8 variants) through the pipeline; the recorded outputs of every forward call are merged by the restatement and
    handed, as a replayed forward, to the SAME decode path without tta: the rows must be equal, row for row"""
    from salsa_amd.crnn.infer import infer_pipelined
    kw = dict(sub_batch=2, n_label_frames=20, decode=decode)
    if chunked:
        kw.update(chunk_len=80, chunk_hop_len=40)
    with torch.no_grad():
        kw['sed_threshold'] = float(torch.quantile(trainer.infer(features[:1])[0].flatten(), 0.7))
    ins, outs = [], []
    rows = infer_pipelined(3, lambda lo, hi: features[lo:hi], ref.recording(trainer.infer, ins, outs), tta=('mic', 'salsa'), **kw)
    assert len(outs) % 8 == 0 and len(outs) // 8 == (3 if chunked else 2)                      # chunks: 4 + 2 and 3 per call
    merged = []
    for c in range(0, len(outs), 8):
        assert all(same_bits(ins[c + v], ref.variant(ins[c], 'mic', v)) for v in range(8))
        group = outs[c:c + 8]
        mp, md = ref.merge([o[0].cpu() for o in group], [o[1].cpu() for o in group], 1, list(range(8)), 'mic', 12)
        merged.append((mp.to(DEV), md.to(DEV)))
    replay = iter(merged)
    want = infer_pipelined(3, lambda lo, hi: features[lo:hi], lambda x: next(replay), **kw)
    assert next(replay, None) is None and rows == want and sum(len(r) for r in rows) > 50


# ---------------------------------------------------------------------------------------------------- 5. the switch
CHILD = """
import os, sys
sys.path[:0] = [{root!r}, {tests!r}]
import torch
import tta_reference as ref
from salsa_amd.crnn import tta
assert os.environ['SALSA_HIP_TTA'] == '0' and not tta.USE_HIP_TTA
x = torch.randn(3, 7, 160, 200, generator=torch.Generator().manual_seed(21)).to('cuda:0')
out = dict()
for name, fmt in (('reg_xyz', 'reg_xyz'), ('accdoa', 'accdoa')):
    p, d = tta.TtaForward([ref.indexing_forward(), ref.equivariant_foa_forward()], 'foa', 'salsa', output_format=fmt)(x)
    out[name] = (p.cpu(), d.cpu())
torch.save(out, {path!r})
"""


def test_switch_off_gives_the_same_tensors_from_the_torch_operators(features, tmp_path):
    """SALSA_HIP_TTA=0 in a fresh process: variants and merge on the torch operators, around forwards that are indexing and
    element-wise arithmetic (indexing_forward) or fixed-order reductions, so both processes see the same forward outputs"""
    from salsa_amd.crnn import tta
    path = str(tmp_path / 'torch_path.pt')
    code = CHILD.format(root=ROOT, tests=os.path.join(ROOT, 'tests'), path=path)
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, SALSA_HIP_TTA='0'), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    theirs = torch.load(path)
    assert tta.USE_HIP_TTA
    for fmt in ('reg_xyz', 'accdoa'):
        p, d = tta.TtaForward([ref.indexing_forward(), ref.equivariant_foa_forward()], 'foa', 'salsa', output_format=fmt)(features)
        assert same_bits(p, theirs[fmt][0]) and same_bits(d, theirs[fmt][1]), fmt
