#!/usr/bin/env python3
"""Timing probe for train(method='COLS') (GPU box): the bound sweep next to reconstruct on the same (n, r, n_p), and a
whole COLS predict on synthetic matrices of the c2- and c3-like shapes.   python tools/cols_probe.py [cells,F,m,r ...]

Prints, per shape: kernel times (HIP events, median of 5) with the bytes each moves, then for one COLS predict the
rounds, sweeps, working-set size, and the time spent in sweeps (incl. the download per round) and in the host QP."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from openmeasure_amd.engine import HipEngine
from openmeasure_amd.sparse_sensing import SPR, DeviceMatrix
from openmeasure_amd.synth import make_R


def timeit(fn, reps=5):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def main():
    shapes = [tuple(int(v) for v in a.split(',')) for a in sys.argv[1:]] or [(1_000_000, 4, 64, 32), (10_000_000, 9, 256, 64)]
    eng = HipEngine()
    for cells, F, m, r in shapes:
        n = cells * F
        X = eng.synth(n, m, 0, cells, eng.to_device(make_R(m, r)), 1e-3, 1)
        spr = SPR(DeviceMatrix(X), F, None, engine=eng)
        spr.fit(select_modes='number', n_modes=r)
        C = spr.optimal_placement()
        spr.train(C)
        Ur, mean, scale = spr._fitted('Ur', 'Ur'), spr._fitted('rowmean', 'X_cnt'), spr._d['scale']
        print(f'cells={cells} F={F} m={m} r={r}  Ur={n * r * 8 / 1e9:.2f} GB')
        lim = eng.to_device(np.stack([np.full(F, -1e3), np.full(F, 1e3)]))
        clamp = eng.to_device(np.full((2, F), np.nan))
        for n_p in (1, 4, 16):
            A = eng.to_device(np.random.default_rng(n_p).standard_normal((n_p, r)))
            out = eng.empty((n_p, n))
            t_r = timeit(lambda: eng.reconstruct(Ur, 0, cells, F, mean, scale, A, out=out))
            t_b = timeit(lambda: eng.bound_sweep(Ur, 0, cells, F, mean, scale, lim, clamp, A, 1e-9, 64))
            rd = n * (8 * r + 8)
            print(f'  n_p={n_p:2d}  reconstruct {t_r:7.3f} ms ({(rd + 8 * n * n_p) / t_r / 1e6:7.1f} GB/s)   '
                  f'bound_sweep {t_b:7.3f} ms ({rd / t_b / 1e6:7.1f} GB/s)   sweep / reconstruct = {t_b / t_r:.2f}')
            del out
        # one COLS predict: a held-out state measured with noise, limits that cut 5 % off each end of the range of the
        # unconstrained reconstruction (so that they bind)
        piv = spr.sensors_
        col = eng.to_host(X[:, m // 2].contiguous()).astype(np.float64)
        rng = np.random.default_rng(3)
        y = np.zeros((len(piv), 3))
        y[:, 0] = col[piv] + 0.05 * np.abs(col[piv]).max() * rng.standard_normal(len(piv))
        y[:, 2] = piv // cells
        a0, _ = spr.predict(y)
        x0 = spr.reconstruct(a0)[:, 0]
        lo = np.array([x0[f * cells:(f + 1) * cells].min() for f in range(F)])
        hi = np.array([x0[f * cells:(f + 1) * cells].max() for f in range(F)])
        del x0, col
        spr.train(C, limits=[lo + 0.05 * (hi - lo), hi - 0.05 * (hi - lo)], method='COLS')
        for rep in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            spr.predict(y)
            dt = time.perf_counter() - t0
        info = spr.cols_info_
        print(f"  COLS predict {1e3 * dt:8.2f} ms: status {info['status']} rounds {info['rounds']} sweeps {info['sweeps']} "
              f"working rows {[len(x) for x in info['rows']]} active {[int(np.count_nonzero(x > 0)) for x in info['multipliers']]} "
              f"max violation {info['max_violation']}  sweeps+downloads {1e3 * info['sweep_seconds']:.2f} ms  host QP "
              f"{1e3 * info['qp_seconds']:.2f} ms")
        del X, Ur, spr
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
