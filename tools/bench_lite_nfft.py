#!/usr/bin/env python
"""SALSA-Lite at n_fft 1024 on one 32 x 60-s batch: the HIP kernel against a torch-composed baseline on the same device (torch.stft in
float64 stored as complex64, log10 of the power, angle of the cross spectra scaled per bin -- the reference's arithmetic, one clip at a
time to bound its float64 temporaries).  hipEvent pairs around each step, `--steps` steps after `--warmup`; one JSON line per arm and one
with the ratio, appended to profiles/lite_nfft_bench.jsonl by the caller."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from salsa_amd.extractor import SalsaExtractor  # noqa: E402
from salsa_amd.synth import synth_clips_device  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--seconds', type=int, default=60)
    ap.add_argument('--n-fft', type=int, default=1024)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    fs, hop, n_fft, n = 24000, 300, a.n_fft, a.seconds * 24000
    audio = synth_clips_device(2600, a.batch, n, device=dev)
    ex = SalsaExtractor(audio_format='mic', feature_type='salsa_lite', n_fft=n_fft, fmax_doa=2000, device=dev)
    _, T, F = ex.output_shape(n)
    out = torch.empty((a.batch, 7, T, F), dtype=torch.float32, device=dev)
    lower, upper, cutoff = 1 if n_fft < 1024 else 2, 2000 * n_fft // fs, 9000 * n_fft // fs
    assert F == cutoff - lower
    win = torch.hann_window(n_fft, periodic=True, dtype=torch.float64, device=dev)
    k = torch.arange(lower, cutoff, dtype=torch.float64, device=dev)
    scale = (1.0 / (2 * math.pi * fs / (n_fft * 343.0) * k)).float()[None, None, :]
    scale[:, :, upper:] = 0
    base = torch.empty_like(out)

    def torch_arm():
        for b in range(a.batch):
            X = torch.stft(audio[b].double(), n_fft, hop, n_fft, win, center=True, pad_mode='reflect', return_complex=True).to(torch.complex64)
            X = X[:, lower:cutoff].permute(0, 2, 1)                                                  # (4, T, F)
            base[b, :4] = 10.0 * torch.log10(torch.clamp(X.real ** 2 + X.imag ** 2, min=1e-10))
            base[b, 4:] = torch.angle(X[1:] * torch.conj(X[:1])) * scale

    hip_ms = timed(lambda: ex.extract(audio, out=out), a.steps, a.warmup)
    torch_ms = timed(torch_arm, a.steps, a.warmup)
    d = (out[:, :, 1:] - base[:, :, 1:]).abs()
    bytes_alg = a.batch * (4 * n * 4 + 7 * T * F * 4)
    for arm, ms in (('hip', hip_ms), ('torch_f64_stft', torch_ms)):
        med = statistics.median(ms)
        print(json.dumps(dict(bench='lite_nfft', arm=arm, device=torch.cuda.get_device_name(0), feature='salsa_lite', n_fft=n_fft, batch=a.batch,
                              seconds=a.seconds, T=T, F=F, steps=a.steps, warmup=a.warmup, ms_median=round(med, 4), ms_min=round(min(ms), 4),
                              ms_max=round(max(ms), 4), algorithmic_bytes=bytes_alg, tb_per_s=round(bytes_alg / med / 1e9, 4),
                              fraction_of_8tbs=round(bytes_alg / med / 1e9 / 8.0, 4))))
    print(json.dumps(dict(bench='lite_nfft', arm='ratio', n_fft=n_fft, torch_over_hip=round(statistics.median(torch_ms) / statistics.median(hip_ms), 2),
                          max_abs_diff_logspec=float(d[:, :4].max()), frac_phase_diff_gt_1e4=float((d[:, 4:] > 1e-4).float().mean()))))


if __name__ == '__main__':
    main()
