"""Times of SPR.assimilate (csrc/assimilate.hip) next to SPR.predict on the device:

    python tools/assimilate_probe.py [--reps 20]

1. The public methods at the placement / predict shapes of BASELINE configs 2 and 3 (s = r = 32 with 4 features, s = r = 64
   with 9; one measurement vector, as bench.py's predict_ms): a small field (2 000 cells per feature -- predict and assimilate
   only see Theta, s x r), QR placement, train(C); then host wall clock per call of predict(y) and of
   assimilate(y, a0, sigma) / assimilate(y, a0, prior_factor=F), uploads and downloads included, and the same assimilate
   with to_host=False.
2. The engine calls alone between device events: solve_ols and solve_pinv (predict's kernels) against assimilate with the
   diagonal and the factor prior, at those shapes and at a tomography-sized s = 4096, r = 32, for 1 and 64 vectors.
One warm-up call, then --reps timed ones: median with min-max."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def wall(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return np.median(out), min(out), max(out)


def events(eng, fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0 = eng.timing_event()
        fn()
        e1 = eng.timing_event()
        torch.cuda.synchronize()
        out.append(eng.elapsed_ms(e0, e1))
    return np.median(out), min(out), max(out)


def fmt(t):
    return f'{t[0]:8.4f} ms (min {t[1]:.4f}, max {t[2]:.4f})'


def public_methods(eng, reps):
    from openmeasure_amd.sparse_sensing import SPR
    for name, F, m, s in (('config 2', 4, 64, 32), ('config 3', 9, 256, 64)):
        rng = np.random.default_rng(s)
        cells = 2000
        X = np.concatenate([(f + 1) * (rng.standard_normal((cells, s)) @ rng.standard_normal((s, m)))
                            + 0.01 * rng.standard_normal((cells, m)) + 10 * f for f in range(F)])
        spr = SPR(X, F, None, engine=eng)
        spr.fit(select_modes='number', n_modes=s)
        C = spr.optimal_placement()
        spr.train(C)
        rows = spr.sensors_
        scl = np.asarray(spr.X_scl)[rows, 0]
        y = np.stack([X[rows, 3] + 0.01 * scl * rng.standard_normal(s), 0.01 * scl, (rows // cells).astype(float)], axis=1)
        a0, sigma = spr.Ar[3] + 0.1 * rng.standard_normal(s), np.full(s, 0.5)
        Fh = spr.assimilate(y, a0, sigma)[2][0]
        print(f'{name}: s = r = {s}, {F} features, one vector; cond(H\') estimate {spr.assimilate_info_["cond"][0]:.2e}')
        print(f'  predict(y)                                  {fmt(wall(lambda: spr.predict(y), reps))}   path {spr.solve_path_}')
        print(f'  assimilate(y, a0, sigma)                    {fmt(wall(lambda: spr.assimilate(y, a0, sigma), reps))}')
        print(f'  assimilate(y, a0, prior_factor=F)           {fmt(wall(lambda: spr.assimilate(y, a0, prior_factor=Fh), reps))}')
        a0_d, sg_d = eng.to_device(a0[None]), eng.to_device(sigma[None])
        print(f'  assimilate(y, a0_dev, sigma_dev, to_host=False) {fmt(wall(lambda: spr.assimilate(y, a0_d, sg_d, to_host=False), reps))}')


def engine_calls(eng, reps):
    for s, r in ((32, 32), (64, 64), (4096, 32), (128, 128)):
        for n_p in (1, 64):
            rng = np.random.default_rng(s + n_p)
            Theta = eng.to_device(rng.standard_normal((s, r)) / np.sqrt(r))
            cnt, scale = eng.to_device(rng.standard_normal(s)), eng.to_device(np.array([1.0, 2.0, 0.5]))
            y = np.stack([rng.standard_normal((n_p, s)), np.full((n_p, s), 0.05), rng.integers(0, 3, (n_p, s)).astype(float)], axis=2)
            y_d, a0 = eng.to_device(y), eng.to_device(rng.standard_normal((n_p, r)))
            S = eng.to_device(rng.uniform(0.3, 2.0, (n_p, r)))
            L = eng.assimilate(Theta, cnt, scale, y_d, a0, S=S)[2].clone()
            print(f's = {s}, r = {r}, n_p = {n_p}:')
            print(f'  solve_ols (predict)        {fmt(events(eng, lambda: eng.solve_ols(Theta, cnt, scale, y_d), reps))}')
            print(f'  solve_pinv (predict)       {fmt(events(eng, lambda: eng.solve_pinv(Theta, cnt, scale, y_d), reps))}')
            print(f'  assimilate, diagonal prior {fmt(events(eng, lambda: eng.assimilate(Theta, cnt, scale, y_d, a0, S=S), reps))}')
            print(f'  assimilate, factor prior   {fmt(events(eng, lambda: eng.assimilate(Theta, cnt, scale, y_d, a0, L=L), reps))}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    from openmeasure_amd.engine import HipEngine
    eng = HipEngine('cuda:0')
    public_methods(eng, args.reps)
    engine_calls(eng, args.reps)


if __name__ == '__main__':
    main()
