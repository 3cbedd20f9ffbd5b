"""GPU tests of the baseline feature kernels (baseline_kernels.hip) off the default settings: every setting of
baseline_families.SETTINGS, on built clips of at most 8000 samples in batches of 3 families, against the float64 restatement
(baseline_reference.py) under base + K * bound -- a tolerance made of the restatement alone (test_baseline_off_default_cpu.py) --
plus the facts that need no tolerance: empty mel rows, digital silence, the GCC peak lag, log rows shared between types, batch
position, repeatability, frame locality and the clip-length edges."""
import functools

import numpy as np
import pytest

import baseline_families as bf
import baseline_reference as br

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


_PLANS = {}


@pytest.fixture(scope='module', autouse=True)
def _release_plans():
    yield
    _PLANS.clear()                                  # (plans are destroyed while the device is still open)


def _ex(name, ft):
    from salsa_amd.baseline_features import BaselineExtractor
    if (name, ft) not in _PLANS:
        _PLANS[name, ft] = BaselineExtractor(feature_type=ft, **bf.keywords(bf.setting(name)[1]))
    return _PLANS[name, ft]


@functools.lru_cache(maxsize=None)
def _reference(name, ft, n, family):
    """(clip, restatement, 1-ulp bound), computed once and left unchanged"""
    cfg = bf.setting(name)[1]
    y = bf.clip(family, n, bf.pad_of(cfg, ft))
    out = y, br.extract(ft, y, *cfg), br.bound(ft, y, *cfg)
    for a in out:
        a.setflags(write=False)
    return out


def _run(name, ft, clips, dev):
    import torch
    return _ex(name, ft).extract(torch.from_numpy(np.stack(clips)).to(dev))


def _zero_lag(F):
    """index of lag 0 among the kept lags cc[-F // 2:] ++ cc[:F // 2] (floor division: ceil(F / 2) negative lags come first)"""
    return (F + 1) // 2


@pytest.mark.parametrize('name', [s[0] for s in bf.SETTINGS])
def test_values_match_the_restatement(dev, name):
    """every (setting, type, length, batch of 3 families): out[i] within base + K * bound of the restatement of clip i, left-out
    share within the cap, empty mel rows exact.  Prints the largest |out - ref| / (base + K * bound) and left-out share per channel
    group of the setting (run with -s)."""
    from salsa_amd import baseline_features as bfeat
    worst = {}
    for nm, cfg, ft, n, fams in bf.entries():
        if nm != name:
            continue
        refs = [_reference(nm, ft, n, f) for f in fams]
        out = _run(nm, ft, [r[0] for r in refs], dev).cpu().numpy()
        shape = bfeat.output_shape(ft, n, cfg[1], cfg[2], cfg[4], cfg[7])
        assert out.shape == (3,) + shape == (3,) + _ex(nm, ft).output_shape(n) and shape[1] == 1 + n // cfg[2]
        wsum = br.row_sums(ft, *cfg)
        empty = wsum == 0
        for i, (fam, (_, ref, bnd)) in enumerate(zip(fams, refs)):
            what = '%s %s N=%d %s' % (nm, ft, n, fam)
            for g, (w, share) in br.compare(out[i], ref, bnd, ft, wsum, what).items():
                worst[g] = max(worst.get(g, (0.0, 0.0)), (w, share))
            # frames 0 and T - 1 are part of the comparison above: the impulses reach them through the reflection alone
            assert (out[i, :4][:, :, empty] == -100.0).all(), what + ': an empty mel row is not exactly -100 dB'
            if ft.endswith('iv'):
                assert (out[i, 4:][:, :, empty] == 0).all(), what + ': an empty mel row has a non-zero IV'
    print(name, {g: 'worst %.3f of the tolerance, left out %.4f' % v for g, v in worst.items()})


@pytest.mark.parametrize('name', [s[0] for s in bf.SETTINGS if len(s[2]) > 1])
def test_log_rows_are_shared_between_the_types(dev, name):
    """the first stage is the same code: the lin types' log rows are bit-equal to each other, and so are the mel types'"""
    import torch
    _, cfg, types = bf.setting(name)
    n = 12 * cfg[2] + cfg[2] // 3
    clips = [bf.clip(f, n, cfg[1]) for f in bf.BATCHES[1]]
    for group in (bf.MEL, bf.LIN):
        outs = [_run(name, ft, clips, dev)[:, :4] for ft in types if ft in group]
        for o in outs[1:]:
            assert torch.equal(o, outs[0]), (name, group)


def test_digital_silence_is_exact(dev):
    """-100 dB, IV 0 and a GCC delta at lag 0, for even and odd F"""
    for name, cfg, types in bf.SETTINGS:
        for ft in types:
            F, n = bf.n_freq(cfg, ft), bf.lengths(cfg, ft)[2]
            out = _run(name, ft, [np.zeros((4, n), np.float32)] * 2, dev).cpu().numpy()
            assert (out[:, :4] == -100.0).all(), (name, ft)
            if ft.endswith('iv'):
                assert (out[:, 4:] == 0).all(), (name, ft)
            elif ft.endswith('gcc'):
                delta = np.zeros(F, np.float32)
                delta[_zero_lag(F)] = 1.0
                np.testing.assert_allclose(out[:, 4:], np.broadcast_to(delta, out[:, 4:].shape), rtol=0, atol=1e-6, err_msg=name + ft)


def test_gcc_peak_sits_at_the_known_delay(dev):
    """delayed noise: the argmax of pair (n, m) is lag d_m - d_n for every F in the list, odd F included; frames whose 2 n_fft
    window touches a clip end are left out"""
    for name, cfg, types in bf.SETTINGS:
        for ft in types:
            if not ft.endswith('gcc'):
                continue
            n, F, hop, n_fft = bf.lengths(cfg, ft)[4], bf.n_freq(cfg, ft), cfg[2], cfg[1]
            out = _run(name, ft, [bf.clip('delayed', n, n_fft)], dev)[0].cpu().numpy()
            clear = [t for t in range(out.shape[1]) if t * hop - n_fft >= 0 and t * hop + n_fft <= n]
            mid = out[4:, clear].mean(axis=1)
            for p, (cn, cm) in enumerate(br.PAIRS):
                assert int(np.argmax(mid[p])) == _zero_lag(F) + bf.DELAYS[cm] - bf.DELAYS[cn], (name, ft, cn, cm)
                assert mid[p].max() > 0.5


@pytest.mark.parametrize('name,ft', bf.INSTANTIATIONS)
def test_batch_position_and_repeat_do_not_matter(dev, name, ft):
    import torch
    cfg = bf.setting(name)[1]
    n = bf.lengths(cfg, ft)[3]
    pad = bf.pad_of(cfg, ft)
    y, a, b = (bf.clip(f, n, pad) for f in ('dc', 'delayed', 'full_scale'))
    alone = _run(name, ft, [y], dev)[0]
    first, last = _run(name, ft, [y, a, b], dev), _run(name, ft, [a, b, y], dev)
    assert torch.equal(first[0], alone) and torch.equal(last[2], alone)
    assert torch.equal(first[1], last[0]) and torch.equal(first[2], last[1])
    assert torch.equal(_run(name, ft, [y, a, b], dev), first)


@pytest.mark.parametrize('name,ft', bf.INSTANTIATIONS)
def test_frames_depend_on_their_own_samples_only(dev, name, ft):
    """frame t of a clip == frame t of the clip with 5 hops of other audio appended, for every t whose window ends before the
    clip's end; == frame t + 5 of the clip with 5 hops prepended, for every t whose window starts at or after the clip's start"""
    import torch
    cfg = bf.setting(name)[1]
    hop, half = cfg[2], bf.pad_of(cfg, ft)
    n = bf.lengths(cfg, ft)[4]
    y, other = bf.clip('silent_middle', n, half, seed=1), bf.clip('dc', 5 * hop, half, seed=2)
    own = _run(name, ft, [y], dev)[0]
    app = _run(name, ft, [np.concatenate([y, other], axis=1)], dev)[0]
    pre = _run(name, ft, [np.concatenate([other, y], axis=1)], dev)[0]
    T = own.shape[1]
    assert app.shape[1] == pre.shape[1] == T + 5
    before_end = [t for t in range(T) if t * hop + half <= n]
    after_start = [t for t in range(T) if t * hop - half >= 0]
    assert len(before_end) >= 6 and len(after_start) >= 6 and 0 in before_end and T - 1 in after_start
    assert torch.equal(app[:, before_end], own[:, before_end])
    assert torch.equal(pre[:, [t + 5 for t in after_start]], own[:, after_start])


@pytest.mark.parametrize('name,ft', bf.INSTANTIATIONS)
def test_shortest_clip(dev, name, ft):
    """N = pad is refused (np.pad's reflection needs N > pad), N = pad + 1 runs"""
    import torch
    cfg = bf.setting(name)[1]
    pad, hop = bf.pad_of(cfg, ft), cfg[2]
    ex = _ex(name, ft)
    with pytest.raises(ValueError):
        ex.extract(torch.zeros((1, 4, pad), dtype=torch.float32, device=dev))
    out = ex.extract(torch.ones((1, 4, pad + 1), dtype=torch.float32, device=dev))
    assert out.shape[2] == 1 + (pad + 1) // hop and bool(torch.isfinite(out).all())
