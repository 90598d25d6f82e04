#!/usr/bin/env python3
"""The three passes of ROM.partial_fit (encode, csrc/validate.hip; subspace_residual and basis_update, csrc/update.hip) and
a whole partial_fit, next to the yardsticks that exist without them, alternating in one process: encode at the same (r, k),
gappy_normal with all rows observed (the kernel the residual pass is modelled on), and -- at the c2-like shape, where both
fit -- fit() of the concatenated m + k matrix, which is what a user without partial_fit has to run.
Shapes: c2-like (1M cells x 4 features = 4M rows, r = 32, k = 64) and c3-like (10M x 9 = 90M rows, r = 64, k = 64).
Per figure: ms (median, min ... max) and the fraction of the one-read bound at 6.3 TB/s -- (8r + 8k + 8) n bytes for encode
and the residual pass, that plus 8 r n written for the update.  Warm-up 2, REPS repetitions.
    python tools/partial_fit_probe.py [--small]"""
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


def wall(fn, reps=REPS, warm=2):
    ts = []
    for _ in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    ts = ts[warm:]
    return float(np.median(ts)), min(ts), max(ts)


def main():
    eng = HipEngine('cuda:0')
    shapes = [(1_000_000, 4, 64, 32, 64, True), (10_000_000, 9, 64, 64, 64, False)]
    if '--small' in sys.argv:
        shapes = [(200_000, 4, 64, 32, 64, True)]
    for cells, F, m, r, k, refit in shapes:
        n = cells * F
        Xall = eng.synth(n, m + k, 0, cells, eng.to_device(make_R(m + k, r, seed=1)), 1e-3, 1) if refit else None
        Xd = Xall[:, :m].contiguous() if refit else eng.synth(n, m, 0, cells, eng.to_device(make_R(m, r, seed=1)), 1e-3, 1)
        Xb = Xall[:, m:] if refit else eng.synth(n, k, 0, cells, eng.to_device(make_R(k, r, seed=2)), 1e-3, 2)
        rom = ROM(DeviceMatrix(Xd), F, None, engine=eng)
        rom.fit(select_modes='number', n_modes=r)
        blk = rom._block()
        ones = torch.ones(n, dtype=torch.uint8, device='cuda:0')
        C = eng.encode(*blk, Xb)
        A, B = eng.to_device(np.eye(r)), eng.to_device(np.zeros((k, r)))
        out = eng.empty((n, r))
        print(f'--- {cells} cells x {F} features = {n} rows, r = {r}, k = {k}')
        res = timeit([lambda: eng.encode(*blk, Xb), lambda: eng.subspace_residual(*blk, Xb, C),
                      lambda: eng.basis_update(*blk, Xb, A, B, out=out),
                      lambda: eng.gappy_normal(*blk, Xb, ones)])
        read = (8 * r + 8 * k + 8) * n
        for name, (t, t0, t1), nbytes in zip(('encode', 'subspace_residual', 'basis_update', 'gappy_normal(ones)'), res,
                                             (read, read, read + 8 * r * n, read + n)):
            bound = nbytes / HBM * 1e3
            print(f'{name:20s} {t:8.3f} ms ({t0:.3f} ... {t1:.3f})  one-read bound {bound:7.3f} ms = {bound / t:4.2f} of it')
        del out
        tw = wall(lambda: rom.partial_fit(Xb))
        print(f'whole partial_fit (fixed rank, host SVD and transfers included): {tw[0]:.3f} ms ({tw[1]:.3f} ... {tw[2]:.3f})'
              f'  last info {rom.partial_fit_info_[-1]}')
        if refit:
            full = ROM(DeviceMatrix(Xall), F, None, engine=eng)
            tf = wall(lambda: (full.fit(select_modes='number', n_modes=r), full._flush_deferred()))
            print(f'fit() of the concatenated {m + k}-column matrix: {tf[0]:.3f} ms ({tf[1]:.3f} ... {tf[2]:.3f})'
                  f'  partial_fit / refit {tw[0] / tf[0]:.2f}')
            del full
        del rom, Xd, Xb, Xall, blk, C
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
