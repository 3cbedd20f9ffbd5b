"""salsa_extract_multichannel (5 - 16 microphones: cov_eig_n_kernel, cyclic complex Jacobi) against the LAPACK reference of
tests/flex_reference.py on the built audio families of tests/flex_families.py: every family, tracking on and off, ew_thresh
1.05 / 4 / 5, the unrolled (6, 8) and the run-time-sized (10, 14, 16) instantiations.  The reference is fed the oracle's STFT of the
same audio; the HIP STFT may differ from it in the last float32 bit, which is what the doubt band M_BAND and the value bound
kappa_c * DELTA_STFT (measured from the reference alone, tests/test_flex_solver_cpu.py) are for."""
import numpy as np
import pytest
import torch

import flex_families as ff
import flex_reference as fr
from test_gpu_parity import ATOL_DB, RTOL

pytestmark = pytest.mark.gpu

CTOR = dict(fs=ff.FS, stft_winsize=512, hop_length=300, fmin_doa=50, fmax_doa=2000, fmax_spec=9000)
SEEDS = (0, 1)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def call_of(thr, trk):
    return dict(clip_freqs=trk, clip_spatial_alias=bool(trk and thr == 4.0), ew_thresh=thr, covmat_avg_neighbours=3, is_tracking=trk,
                floor_mask_ratio=1.5)


@pytest.mark.parametrize('name', sorted(ff.AUDIO_FAMILIES))
def test_multichannel_against_lapack_reference_on_audio_family(dev, oracle, name):
    from salsa_amd.flexible import SalsaFeatures
    sf = SalsaFeatures(**CTOR)
    gated = excluded = 0
    cache = {}
    for fam, n_ch, thr, trk in ff.audio_cases():
        if fam != name:
            continue
        if n_ch not in cache:
            ys = np.stack([ff.audio(name, n_ch, seed) for seed in SEEDS])
            Xs = [np.stack([oracle.stft(y[c], CTOR['stft_winsize'], CTOR['hop_length']) for c in range(n_ch)]) for y in ys]
            cache[n_ch] = (ys, torch.from_numpy(ys).to(dev), Xs, [fr.decompose(X, 3) for X in Xs])
        ys, a, Xs, decs = cache[n_ch]
        call = call_of(thr, trk)
        o1 = sf.extract_batch(a, **call)
        o2 = sf.extract_batch(a, **call)
        assert torch.equal(o1, o2), 'two calls on the same buffer differ'
        out = o1.cpu().numpy()
        assert out.shape[:2] == (len(SEEDS), 2 * n_ch - 1)
        for i in range(len(SEEDS)):
            ref = fr.features(Xs[i], decs[i], CTOR, call)
            F, T = ref['gate'].shape
            real_tf = fr.real_spectrum_bins(F, T, ref['lo'], CTOR['stft_winsize'], ys.shape[2], CTOR['hop_length'])
            what = '%s n_ch %d thresh %g tracking %s clip %d' % (name, n_ch, thr, trk, i)
            np.testing.assert_allclose(out[i, :n_ch], ref['spec_db'], rtol=RTOL, atol=ATOL_DB, err_msg=what)
            st = fr.compare(out[i, n_ch:], ref, real_tf, trk, what=what, silent_exact=False)
            share = st['in_band'] / max(1, st['compared'])
            print('%-50s: %6d bins compared, %d in the doubt band (%.1e), %7d gated elements, %d left out, worst |dphase| %.2e rad '
                  '= %.3f of its bound; %.4f of %d silent-only passing bins show'
                  % (what, st['compared'], st['in_band'], share, st['gated'], st['excluded'], st['max_err'], st['worst'], st['silent_shown'], st['hidden']))
            assert share <= fr.DOUBT_SHARE_MAX, what
            gated += st['gated']
            excluded += st['excluded']
    if name == 'silent_ch0':
        assert gated == 0
    else:
        assert gated > 1000 and excluded <= fr.EXCLUDED_SHARE_MAX * gated, (name, gated, excluded)
