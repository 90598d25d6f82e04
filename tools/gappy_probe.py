#!/usr/bin/env python3
"""gappy_normal (csrc/gappy.hip) next to encode (csrc/validate.hip, the yardstick) at the same shape, alternating in one
process: c3-like (10M cells x 9 features, r = 64), c2-like (1M x 4, r = 32) and 1M x 8 at r = 128; k = 1, 16, 64; masks: all
ones, one feature of F, 1 % random rows (which skips almost no panel: the honest worst case for skipping).  Per figure: ms
(median, min ... max), the fraction of the one-read bound (8r + 8k + 1) n_touched bytes at 6.3 TB/s, TFLOP/s of
2 n_obs r (r + k).  Then one whole ROM.gappy_transform (k = 16, one-feature mask, downloads and host solve included) at the
c2-like shape.  Warm-up 2, REPS repetitions.   python tools/gappy_probe.py [--small]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from openmeasure_amd.engine import HipEngine  # noqa: E402
from openmeasure_amd.rom import DeviceMatrix  # noqa: E402
from openmeasure_amd.sparse_sensing import ROM  # noqa: E402
from openmeasure_amd.synth import make_R  # noqa: E402

REPS = 7
HBM = 6.3e12


def timeit(fns, reps=REPS, warm=2):
    """the functions alternate inside every repetition -> [(median, min, max)] in ms"""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out[i].append(e0.elapsed_time(e1))
    return [(float(np.median(o)), min(o), max(o)) for o in out]


def main():
    eng = HipEngine('cuda:0')
    shapes = [(1_000_000, 4, 64, 32), (10_000_000, 9, 64, 64), (1_000_000, 8, 160, 128)]
    if '--small' in sys.argv:
        shapes = [(200_000, 4, 64, 32)]
    for cells, F, m, r in shapes:
        n = cells * F
        Xd = eng.synth(n, m, 0, cells, eng.to_device(make_R(m, r, seed=1)), 1e-3, 1)
        rom = ROM(DeviceMatrix(Xd), F, None, engine=eng)
        rom.fit(select_modes='number', n_modes=r)
        Ur, mean, scale = rom._d['Ur'], rom._d['rowmean'], rom._d['scale']
        masks = {'ones': torch.ones(n, dtype=torch.uint8, device='cuda:0'),
                 'feature': torch.zeros(n, dtype=torch.uint8, device='cuda:0'),
                 'random1%': (torch.rand(n, device='cuda:0') < 0.01).to(torch.uint8)}
        masks['feature'][cells:2 * cells] = 1
        print(f'--- {cells} cells x {F} features = {n} rows, r = {r}')
        for k in (1, 16, 64):
            Xk = Xd[:, :k]
            for name, md in masks.items():
                n_obs = int(md.sum())
                panels = int((md.view(-1)[:n - n % 64].view(-1, 64).any(dim=1)).sum()) + (1 if n % 64 else 0)
                touched = min(n, panels * 64)
                (tg, tg0, tg1), (te, te0, te1) = timeit([
                    lambda: eng.gappy_normal(Ur, 0, cells, F, mean, scale, Xk, md),
                    lambda: eng.encode(Ur, 0, cells, F, mean, scale, Xk)])
                bound = ((8 * r + 8 * k) * touched + n) / HBM * 1e3
                print(f'k={k:3d} {name:9s} gappy {tg:8.3f} ms ({tg0:.3f} ... {tg1:.3f})  encode {te:8.3f} ms ({te0:.3f} ... {te1:.3f})'
                      f'  gappy/encode {tg / te:5.2f}  one-read bound {bound:7.3f} ms = {bound / tg:4.2f} of it'
                      f'  {2.0 * n_obs * r * (r + k) / (tg * 1e-3) / 1e12:6.2f} TFLOP/s  panels read {panels}/{-(-n // 64)}')
        if (cells, F) == (shapes[0][0], shapes[0][1]):
            Xo = Xd[:, :16]
            ts = []
            for _ in range(2 + REPS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rom.gappy_transform(Xo, masks['feature'])
                ts.append(1e3 * (time.perf_counter() - t0))
            ts = ts[2:]
            print(f'whole gappy_transform, k = 16, one-feature mask: {np.median(ts):.3f} ms ({min(ts):.3f} ... {max(ts):.3f})', rom.gappy_info_['passes'], 'pass')
        del rom, Xd


if __name__ == '__main__':
    main()
