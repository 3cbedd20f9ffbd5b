#!/usr/bin/env python
"""The deviation of salsa_nn_seld_score's distance statement (salsa_nn_seld_distance: seld_score.h's distance_deg on the device) from
crnn/metrics.py::angular_distance_deg over ALL 181 x 181 x 361 integer (elevation 1, elevation 2, |azimuth difference|) triples.
crnn/score.py's DEFAULT_MARGIN is at least 16 times the worst difference this prints.  Run once on the GPU:

    python tools/probe_score_distance.py [--out profiles/seld_score_distance.txt]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from salsa_amd import _lib
    from salsa_amd.crnn.metrics import angular_distance_deg
    from salsa_amd.crnn.score import DEFAULT_MARGIN
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'seld_score_distance.txt'))
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    L = _lib.load()
    ele2, dazi = (a.reshape(-1) for a in np.meshgrid(np.arange(-90, 91), np.arange(0, 361), indexing='ij'))
    worst, worst_at, n, n_diff, worst_near_20 = 0.0, None, 0, 0, 0.0
    for ele1 in range(-90, 91):
        q = np.stack([np.zeros_like(ele2), np.full_like(ele2, ele1), dazi, ele2], axis=1).astype(np.int16)
        quads = torch.from_numpy(q).to(dev)
        out = torch.empty((len(q),), dtype=torch.float64, device=dev)
        rc = L.salsa_nn_seld_distance(C.c_void_p(quads.data_ptr()), len(q), C.c_void_p(out.data_ptr()),
                                      C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        assert rc == 0, rc
        ref = angular_distance_deg(0, ele1, dazi, ele2)
        got = out.cpu().numpy()
        err = np.abs(got - ref)
        k = int(err.argmax())
        if err[k] > worst:
            worst, worst_at = float(err[k]), (ele1, int(ele2[k]), int(dazi[k]), float(ref[k]), float(got[k]))
        near = np.abs(ref - 20) < 1
        worst_near_20 = max(worst_near_20, float(err[near].max()) if near.any() else 0.0)
        n += len(q)
        n_diff += int((got != ref).sum())
    lines = ['salsa_nn_seld_distance against crnn/metrics.py::angular_distance_deg on %s (numpy %s)' % (torch.cuda.get_device_name(0), np.__version__),
             'triples (ele1, ele2, |dazi|): %d, of which %d differ in any bit' % (n, n_diff),
             'worst |device - host|: %.6e degrees at ele1 %d ele2 %d dazi %d (host %.17g, device %.17g)' % ((worst,) + worst_at),
             'worst |device - host| where the distance is within 1 degree of 20: %.6e degrees' % worst_near_20,
             '16 x worst: %.6e degrees; DEFAULT_MARGIN %.6e degrees (%s)' % (16 * worst, DEFAULT_MARGIN, 'holds' if DEFAULT_MARGIN >= 16 * worst else 'TOO SMALL')]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
