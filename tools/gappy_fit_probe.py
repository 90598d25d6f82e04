#!/usr/bin/env python3
"""ROM.fit_gappy at BASELINE config 3 (10M cells x 9 features x 256 snapshots f64 = 184 GB, 64 modes, uint8 mask 23 GB)
with 5 % random holes -- the largest BASELINE shape whose X, basis and mask fit in HBM together.  Meant to run under
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python3 tools/gappy_fit_probe.py fit`.

  fit          one fit_gappy(max_iter=2) (row fill, 3 fits, 2 fill passes), then the fill pass and the row fill alone, timed
               with stream events (REPS repetitions), against the traffic model of DESIGN.md:
                 n m mask bytes + 8 r per (row, slice of A) with a hole + 16 bytes per hole
               and the same with whole 64-byte sectors per run of holes (what HBM moves for scattered 8-byte accesses).
  reconstruct  the yardstick in a process of its own (its (m, n) output is as large as X): one reconstruct of m = 256
               vectors at the same n and r on a random basis.
  --small      1/100 of the cells (a smoke run of this script)."""
import os
import sys
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from openmeasure_amd.engine import HipEngine  # noqa: E402
from openmeasure_amd.rom import DeviceMatrix  # noqa: E402
from openmeasure_amd.sparse_sensing import ROM  # noqa: E402
from openmeasure_amd.synth import make_R  # noqa: E402

REPS = 3
CHUNK = 2_000_000


def timed(fn, reps=REPS):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out)), min(out), max(out)


def main():
    cells = 100_000 if '--small' in sys.argv else 10_000_000
    F, m, r = 9, 256, 64
    n = cells * F
    eng = HipEngine('cuda:0')
    if 'reconstruct' in sys.argv:
        Ur = eng.empty((n, r))
        for i0 in range(0, n, CHUNK):
            Ur[i0:i0 + CHUNK].normal_()
        mean, scale, A = eng.zeros((n,)), eng.to_device(np.ones(F)), eng.to_device(np.random.default_rng(0).standard_normal((m, r)))
        out = eng.empty((m, n))
        eng.reconstruct(Ur, 0, cells, F, mean, scale, A, out=out)
        t = timed(lambda: eng.reconstruct(Ur, 0, cells, F, mean, scale, A, out=out))
        print(f'reconstruct of {m} vectors, n = {n}, r = {r}: {t[0]:.2f} ms ({t[1]:.2f} ... {t[2]:.2f}), '
              f'{(8 * r * n * -(-m // 16) + 8 * m * n) / t[0] / 1e9:.2f} TB/s of 8 r n per 16 vectors + 8 m n written')
        return
    Xd = eng.synth(n, m, 0, cells, eng.to_device(make_R(m, r, seed=1)), 1e-3, 1)
    M = torch.empty((n, m), dtype=torch.uint8, device='cuda:0')
    holes = rows_sl = sectors = 0
    sl = min(256, 8192 // r)
    for i0 in range(0, n, CHUNK):
        h = torch.rand((min(CHUNK, n - i0), m), device='cuda:0') < 0.05
        M[i0:i0 + CHUNK] = (~h).to(torch.uint8)
        holes += int(h.sum())
        for j0 in range(0, m, sl):
            rows_sl += int(h[:, j0:j0 + sl].any(dim=1).sum())
        sectors += int(h.view(h.shape[0], m // 8, 8).any(dim=2).sum())         # 64-byte sectors of X that hold a hole
        del h
    print(f'n = {n}, m = {m}, r = {r}: {holes} holes ({100.0 * holes / (n * m):.2f} %), {rows_sl} (row, slice) pairs with a hole '
          f'of {n * -(-m // sl)}, slice = {sl} columns, {sectors} sectors with a hole')
    rom = ROM(DeviceMatrix(Xd), F, None, engine=eng)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rom.fit_gappy(M, max_iter=2, select_modes='number', n_modes=r)
        e1.record()
        torch.cuda.synchronize()
    print(f'fit_gappy(max_iter=2): {e0.elapsed_time(e1):.1f} ms', rom.gappy_fit_info_)
    A_d = eng.to_device(np.ascontiguousarray(rom.Ar))
    Ur, mean, scale = rom._d['Ur'], rom._d['rowmean'], rom._d['scale']
    t = timed(lambda: eng.gappy_fill(Ur, 0, cells, F, mean, scale, A_d, Xd, M))
    model = n * m + 8 * r * rows_sl + 16 * holes
    moved = n * m + 8 * r * rows_sl + 128 * sectors
    print(f'gappy_fill: {t[0]:.2f} ms ({t[1]:.2f} ... {t[2]:.2f}); traffic model {model / 1e9:.1f} GB = {model / t[0] / 1e9:.2f} TB/s; '
          f'with whole sectors {moved / 1e9:.1f} GB = {moved / t[0] / 1e9:.2f} TB/s; {2.0 * holes * r / t[0] / 1e9:.2f} TFLOP/s')
    t = timed(lambda: eng.gappy_rowfill(Xd, 0, M))
    print(f'gappy_rowfill (two sweeps): {t[0]:.2f} ms ({t[1]:.2f} ... {t[2]:.2f}); 2 (n m + 8 n m) = {18.0 * n * m / 1e9:.1f} GB = '
          f'{18.0 * n * m / t[0] / 1e9:.2f} TB/s')
    print(f'peak allocated {torch.cuda.max_memory_allocated() / 1e9:.1f} GB')


if __name__ == '__main__':
    main()
