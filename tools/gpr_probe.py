"""Times of the Gaussian-process kernels (csrc/gp.hip) on the device:

    python tools/gpr_probe.py [--reps 5] [--no-oracle]
    python tools/gpr_probe.py --ard [--reps 5]

train at m = 256 / r = 64 and m = 512 / r = 128 with a fixed 200 evaluations (rel_error = 0), predict at n_p = 1000.
Per shape: ms per evaluation (the launch divided by the 201 factorisations it makes: 200 with a step and one at the
parameters kept) and the f64 rate against m^3 flops per evaluation and mode; for predict, ms per call.  One warm-up launch,
then --reps timed ones between device events: median, minimum and maximum are printed.  As context, the NumPy oracle
(tests/test_gpr_host.py, LAPACK route) for ONE mode and 20 evaluations on this host, scaled to the same work.

--ard: the ARD + output-scale training kernel (gp_train_ard, flags = 3) next to the plain one (gp_train) in the same process, at
m = 130 and m = 530 with d = 3, r = 64 and 100 evaluations with a step: after one warm-up launch of each, --reps pairs of
launches that alternate plain / flagged.  Per kernel: evaluations per second (modes x 101 factorisations / time), median with
min-max; the ratio flagged / plain of the medians and the min-max of the per-pair ratios.  The flagged kernel adds O(m^2 d)
work per evaluation (the scaled distances, twice) to m^3."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(eng, fn, reps):
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


def ard_against_plain(eng, reps):
    import torch
    from tests.test_gpr_host import gp_case
    n_eval, r, d, flags = 100, 64, 3, 3
    for m in (130, 530):
        P0, Y = gp_case(m, d, r, seed=m, noise=0.3)
        P0_d, Y_d = eng.to_device(P0), eng.to_device(Y)
        raw3, rawn = eng.zeros((r, 3)), eng.zeros((r, eng.gp_n_par(d, flags)))
        runs = {'plain': lambda: eng.gp_train(P0_d, Y_d, 'matern52', raw3, 0.1, n_eval, 0.0),
                'flagged': lambda: eng.gp_train_ard(P0_d, Y_d, 'matern52', flags, rawn, 0.1, n_eval, 0.0)}
        ms = {k: [] for k in runs}
        for k, fn in runs.items():
            info = eng.to_host(fn()[3])
            assert np.all(info[:, 0] == n_eval) and np.all(info[:, 3] == 0), (k, info[:, :4])
        torch.cuda.synchronize()
        for _ in range(reps):
            for k, fn in runs.items():
                e0 = eng.timing_event()
                fn()
                e1 = eng.timing_event()
                torch.cuda.synchronize()
                ms[k].append(eng.elapsed_ms(e0, e1))
        rate = {k: r * (n_eval + 1) / (np.array(v) * 1e-3) for k, v in ms.items()}
        for k, v in rate.items():
            print(f'{k:8s} m={m} d={d} r={r}: {np.median(v):10.0f} evaluations/s (min {v.min():.0f}, max {v.max():.0f}; {reps} reps), '
                  f'{np.median(ms[k]):.2f} ms per launch')
        pair = rate['flagged'] / rate['plain']
        print(f'ratio    m={m}: flagged / plain = {np.median(rate["flagged"]) / np.median(rate["plain"]):.3f} of the medians '
              f'(per pair {pair.min():.3f} to {pair.max():.3f}); roughly (2 d + 8) m^2 more operations next to m^3: {(2 * d + 8) / m:.3f}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-oracle', action='store_true')
    ap.add_argument('--ard', action='store_true', help='time the ARD + output-scale kernel next to the plain one')
    args = ap.parse_args()
    from openmeasure_amd.engine import HipEngine
    if args.ard:
        return ard_against_plain(HipEngine('cuda:0'), args.reps)
    from tests.test_gpr_host import gp_case, gp_distance, gp_train
    eng = HipEngine('cuda:0')
    n_eval = 200
    for m, r in ((256, 64), (512, 128)):
        P0, Y = gp_case(m, 3, r, seed=m, noise=0.3)
        P0_d, Y_d, raw0 = eng.to_device(P0), eng.to_device(Y), eng.zeros((r, 3))
        state = {}

        def train():
            state['out'] = eng.gp_train(P0_d, Y_d, 'matern52', raw0, 0.1, n_eval, 0.0)
        med, lo, hi = timed(eng, train, args.reps)
        raw, Kinv, alpha, info, _ = state['out']
        info = eng.to_host(info)
        assert np.all(info[:, 0] == n_eval) and np.all(info[:, 3] == 0), info[:, :4]
        per = med / (n_eval + 1)
        print(f'train   m={m} r={r}: {med:9.2f} ms per launch (min {lo:.2f}, max {hi:.2f}; {args.reps} reps) = {per:.4f} ms per '
              f'evaluation of all modes, {r * m ** 3 / (per * 1e-3) / 1e12:.3f} Tflop/s f64 against m^3 per evaluation and mode')
        Ps = eng.to_device(np.random.default_rng(0).standard_normal((1000, 3)))
        med, lo, hi = timed(eng, lambda: eng.gp_predict(P0_d, Ps, 'matern52', raw, Kinv, alpha), args.reps)
        print(f'predict m={m} r={r} n_p=1000: {med:.3f} ms (min {lo:.3f}, max {hi:.3f}), '
              f'{2 * 1000 * r * m * m / (med * 1e-3) / 1e12:.3f} Tflop/s f64 against 2 m^2 per point and mode')
        if not args.no_oracle:
            D = gp_distance(P0)
            t0 = time.perf_counter()
            gp_train(D, Y[:, 0], 'matern52', max_iter=20, tol=0.0, route='inv')
            dt = (time.perf_counter() - t0) / 20
            print(f'oracle  m={m}: {1e3 * dt:.2f} ms per evaluation of ONE mode on this host (NumPy, LAPACK route) = '
                  f'{1e3 * dt * r:.1f} ms for {r} modes')


if __name__ == '__main__':
    main()
