#!/usr/bin/env python3
"""bound_sweep next to bound_sweep_batch on the same vectors (n_p = 16, 32, 48, 64, 256; 32 and 48 bracket _cpod.BATCH_FROM)
and one whole ROM.CPOD call, in one process, at the c2-like (1M cells x 4 features, r = 32) and c3-like (10M x 9, r = 64) shapes of tools/cols_probe.py.
Warm-up, REPS repetitions, median and min ... max per figure.   python tools/cpod_probe.py [--small]"""
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


def timeit(fn, reps=REPS, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return np.median(out), min(out), max(out)


def main():
    eng = HipEngine('cuda:0')
    shapes = [(1_000_000, 4, 64, 32), (10_000_000, 9, 128, 64)]
    if '--small' in sys.argv:
        shapes = [(200_000, 4, 64, 32)]
    for cells, F, m, r in shapes:
        n = cells * F
        Xd = eng.synth(n, m, 0, cells, eng.to_device(make_R(m, r, seed=1)), 1e-3, 1)
        rom = ROM(DeviceMatrix(Xd), F, None, engine=eng)
        rom.fit(select_modes='number', n_modes=r)
        Ur, mean, scale = rom._d['Ur'], rom._d['rowmean'], rom._d['scale']
        mm = eng.to_host(eng.feature_minmax(Xd, 0, cells, F))
        lo, hi = mm[:, 0], mm[:, 1]
        lim = eng.to_device(np.stack([lo, hi]))
        clamp = eng.to_device(np.full((2, F), np.nan))
        rng = np.random.default_rng(0)
        Ar = np.asarray(rom.Ar)
        for n_p in (16, 32, 48, 64, 256):
            A = eng.to_device(Ar[rng.integers(0, m, n_p)] * (1 + 0.01 * rng.standard_normal((n_p, 1))))
            t_o = timeit(lambda: eng.bound_sweep(Ur, 0, cells, F, mean, scale, lim, clamp, A, 1e-9, 64))
            t_b = timeit(lambda: eng.bound_sweep_batch(Ur, 0, cells, F, mean, scale, lim, clamp, A, 1e-9, 64))
            flop = 2.0 * n * r * n_p
            passes_o, passes_b = -(-n_p // 16), -(-n_p // 64)
            rd = n * (8 * r + 8)
            print(f'n={n} r={r} n_p={n_p:4d}  bound_sweep {t_o[0]:8.3f} ms ({t_o[1]:.3f} ... {t_o[2]:.3f}; '
                  f'{flop / t_o[0] / 1e9:5.1f} TFLOP/s, {passes_o * rd / t_o[0] / 1e6:6.0f} GB/s)   '
                  f'bound_sweep_batch {t_b[0]:8.3f} ms ({t_b[1]:.3f} ... {t_b[2]:.3f}; {flop / t_b[0] / 1e9:5.1f} TFLOP/s, '
                  f'{passes_b * rd / t_b[0] / 1e6:6.0f} GB/s)   old / batch = {t_o[0] / t_b[0]:.2f}', flush=True)
        # whole CPOD: limits that cut 2 % off each end of every feature's range
        limits = [lo + 0.02 * (hi - lo), hi - 0.02 * (hi - lo)]
        for rep in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            try:
                rom.CPOD({'limits': limits})
            except RuntimeError as e:
                print('  CPOD:', e, flush=True)
                break
            dt = time.perf_counter() - t0
            info = rom.cpod_info_
            st = info['status']
            print(f'  CPOD m={m} call {rep}: {dt:.3f} s  sweeps {info["sweeps"]} rounds max {max(info["rounds"])} '
                  f'working rows max {max(len(x) for x in info["rows"])} cached rows {info["cached_rows"]}  '
                  f'sweep+download {info["sweep_seconds"]:.3f} s  rows {info["rows_seconds"]:.3f} s  host QP {info["qp_seconds"]:.3f} s  '
                  f'ols/optimal/infeasible {st.count("ols")}/{st.count("optimal")}/{st.count("infeasible")}', flush=True)
        del rom, Xd, Ur
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
