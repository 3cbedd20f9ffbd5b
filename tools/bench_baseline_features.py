#!/usr/bin/env python
"""Time the baseline SELD features (salsa_amd/baseline_features.py) on one MI355X: for each type, a batch of 32 x 60-s 4-channel
clips resident in HBM -> one JSON line with ms per batch, audio-s/s, the algorithmic bytes (audio read once + features written
once) and their fraction of 8 TB/s, and a torch-composed baseline on the same GPU (torch.stft in float64, matmul, torch.fft.irfft)
with the HIP path's speed-up over it.

    python tools/bench_baseline_features.py [--clips 32] [--seconds 60] [--steps 20] [--warmup 3] [--types melspec,...]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from salsa_amd import baseline_features as bf  # noqa: E402
from salsa_amd.extractor import compress_matrix  # noqa: E402
from salsa_amd.synth import synth_clips_device  # noqa: E402

PEAK = 8e12


def torch_composed(ft, audio, n_fft=512, hop=300, n_mels=128, fmin=50, fmax=12000):
    """the same features from stock torch ops (float64 STFT stored as complex64, float32 rest)"""
    B, _, N = audio.shape
    dev = audio.device
    W = torch.from_numpy(compress_matrix(n_fft) if ft.startswith('lin') else bf.mel_matrix(24000, n_fft, n_mels, fmin, fmax)).to(dev)
    y = audio.reshape(B * 4, N).double()

    def stft(n):
        win = torch.zeros(n, dtype=torch.float64, device=dev)
        win[(n - n_fft) // 2:(n - n_fft) // 2 + n_fft] = torch.hann_window(n_fft, periodic=True, dtype=torch.float64, device=dev)
        X = torch.stft(y, n, hop, n, window=win, center=True, pad_mode='reflect', return_complex=True)
        return X.to(torch.complex64).reshape(B, 4, n // 2 + 1, -1)   # [B, 4, bins, T]
    X = stft(n_fft)
    p = X.real * X.real + X.imag * X.imag
    rows = [10.0 * torch.log10(torch.clamp(torch.matmul(W, p), min=1e-10)).transpose(-1, -2)]     # [B, 4, T, F]
    if ft.endswith('iv'):
        iv = (X[:, :1].conj() * X[:, 1:]).real
        iv = iv / (torch.sqrt((iv * iv).sum(dim=1, keepdim=True)) + 1e-8)
        rows.append(torch.matmul(W, iv).transpose(-1, -2))
    elif ft.endswith('gcc'):
        n2 = 2 * n_fft
        X2 = stft(n2)
        F = W.shape[0]
        lags = torch.from_numpy(bf.gcc_lags(F, n2)).to(dev)
        R = torch.stack([X2[:, m] * X2[:, n].conj() for n, m in bf.PAIRS], dim=1)
        cc = torch.fft.irfft(torch.exp(1j * torch.angle(R)), n=n2, dim=2)          # [B, 6, n2, T]
        rows.append(cc.index_select(2, lags).transpose(-1, -2))
    return torch.cat(rows, dim=1)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--clips', type=int, default=32)
    ap.add_argument('--seconds', type=float, default=60.0)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--torch-steps', type=int, default=3)
    ap.add_argument('--types', default=','.join(bf.FEATURE_TYPES))
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    N = int(a.seconds * 24000)
    audio = synth_clips_device(1000, a.clips, n_samples=N, device=dev)
    for ft in a.types.split(','):
        ex = bf.BaselineExtractor(feature_type=ft, n_mels=128, fmin=50, fmax=12000, device=dev)
        out = ex.extract(audio)
        ms = timed(lambda: ex.extract(audio, out=out), a.steps, a.warmup)
        nbytes = audio.numel() * 4 + out.numel() * 4
        ref = torch_composed(ft, audio)
        err = float((ref - out).abs().max())
        del ref
        torch.cuda.empty_cache()
        ms_t = timed(lambda: torch_composed(ft, audio), a.torch_steps, 1)
        print(json.dumps({'metric': 'baseline_features', 'feature_type': ft, 'clips': a.clips, 'seconds': a.seconds,
                          'shape': list(out.shape), 'ms_per_batch': round(ms, 4), 'audio_s_per_s': round(a.clips * a.seconds / ms * 1e3, 1),
                          'algorithmic_bytes': nbytes, 'fraction_of_8TBps': round(nbytes / (ms * 1e-3) / PEAK, 4),
                          'torch_composed_ms': round(ms_t, 3), 'speedup_vs_torch': round(ms_t / ms, 2),
                          'max_abs_diff_vs_torch': round(err, 6), 'device': torch.cuda.get_device_name(0)}), flush=True)
        del out, ex
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
