"""predict() on a wide basis (r > 128): the normal-equations workspace kernel (solve_ols_wide_kernel) and the SVD (pinv)
workspace kernel (solve_pinv_wide_kernel), one vector, s = r, between device events:

    python tools/wide_predict_probe.py [--reps 5] [--widths 200 300 600 1024]

One warm-up call, then --reps timed ones: median with min-max."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.assimilate_probe import events, fmt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--widths', type=int, nargs='+', default=[200, 300, 600, 1024])
    args = ap.parse_args()
    from openmeasure_amd.engine import HipEngine
    eng = HipEngine('cuda:0')
    rng = np.random.default_rng(0)
    for r in args.widths:
        s = r
        Theta = np.linalg.qr(rng.standard_normal((s, r)))[0] * np.logspace(0, -1, r)
        y = np.zeros((1, s, 3))
        y[0, :, 0] = rng.standard_normal(s)
        dev = (eng.to_device(Theta), eng.to_device(np.zeros(s)), eng.to_device(np.ones(1)), eng.to_device(y))
        print(f's = {s}, r = {r}, n_p = 1:')
        print(f'  solve_ols, workspace kernel  {fmt(events(eng, lambda: eng.solve_ols(*dev), args.reps))}')
        print(f'  solve_pinv, workspace kernel {fmt(events(eng, lambda: eng.solve_pinv(*dev), args.reps))}')


if __name__ == '__main__':
    main()
