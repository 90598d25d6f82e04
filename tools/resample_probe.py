#!/usr/bin/env python3
"""Time the resampling of a snapshot matrix from a point cloud onto a voxel grid: a jittered 128^3 source cloud onto a 128^3
VoxelGrid, 4 features, m = 256 snapshots, float64.  Warm-up 2, 7 repetitions; per step (bin, sort, search, apply) the median
with min - max from stream events, for 'nearest' and for 'idw' with k = 8; the candidates inspected per target; for apply the
effective TB/s (bytes of the rows read plus the rows written) next to what a user can do today with torch on the same
tensors: index_select for 'nearest', the loop out += w[:, j, None] * X[idx[:, j]] for 'idw'.  The search is reported next to
scipy's cKDTree(...).query(..., workers=16) on the same points, for orientation only.

    python tools/resample_probe.py [--cells 128] [--features 4] [--m 256] [--dtype f64] [--reps 7] [--warmup 2] [--no-scipy]

Prints one JSON line per method."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STEPS = ('bin', 'sort', 'search', 'apply', 'torch')


def stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cells', type=int, default=128)
    ap.add_argument('--features', type=int, default=4)
    ap.add_argument('--m', type=int, default=256)
    ap.add_argument('--dtype', choices=('f64', 'f32'), default='f64')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--no-scipy', action='store_true')
    args = ap.parse_args()
    import torch
    from openmeasure_amd.engine import HipEngine
    from openmeasure_amd.utils import VoxelGrid

    eng = HipEngine('cuda:0')
    n, F, m = args.cells, args.features, args.m
    grid = VoxelGrid((0.0, 0.0, 0.0), (1.0 / n,) * 3, (n, n, n))
    rng = np.random.default_rng(0)
    xyz = grid.cell_centers() + (rng.random((n ** 3, 3)) - 0.5) * (0.9 / n)     # every source within 0.45 cells of a centre
    xyz = xyz[rng.permutation(len(xyz))]                                         # ... in no particular order
    n_src = n_dst = n ** 3
    dtype = torch.float64 if args.dtype == 'f64' else torch.float32
    X = torch.randn((F * n_src, m), dtype=dtype, device=eng.device)
    out = torch.empty((F * n_dst, m), dtype=dtype, device=eng.device)
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    nb = eng.resample_bin_counts(lo, hi, n_src)
    src = eng.to_device(xyz)
    esz = X.element_size()

    def event():
        return eng.timing_event()

    for method, k in (('nearest', 1), ('idw', 8)):
        ms = {s: [] for s in STEPS}
        for rep in range(args.warmup + args.reps):
            ev = {s: eng.time_next('resample_' + s) for s in ('bin', 'apply')}
            ev['search'] = eng.time_next('resample_knn')
            key = eng.resample_bin(src, nb, lo, hi)
            s0 = event()
            perm = torch.sort(key, stable=True)[1]
            start, _ = eng._exclusive_scan(torch.bincount(key, minlength=nb[0] * nb[1] * nb[2]))
            src_sorted = src.index_select(0, perm).contiguous()
            s1 = event()
            idx, d2, w, seen = eng.resample_knn(src_sorted, perm, start, nb, lo, hi, grid, k, method, None)
            eng.resample_apply(X, n_src, F, idx, w, method, 0.0, out=out)
            t0 = event()
            X3 = X.view(F, n_src, m)
            if method == 'nearest':
                ref = torch.index_select(X3, 1, idx[:, 0])
            else:
                ref = torch.zeros((F, n_dst, m), dtype=dtype, device=eng.device)
                for j in range(k):
                    ref += w[:, j, None].to(dtype) * X3[:, idx[:, j]]
            t1 = event()
            torch.cuda.synchronize()
            if rep >= args.warmup:
                for s in ('bin', 'search', 'apply'):
                    ms[s].append(eng.elapsed_ms(*ev[s]))
                ms['sort'].append(eng.elapsed_ms(s0, s1))
                ms['torch'].append(eng.elapsed_ms(t0, t1))
            if rep == 0:                                      # the yardstick computes the same thing
                a, b = out[:4096].double(), ref.view(F * n_dst, m)[:4096].double()
                agree = bool((a == b).all()) if method == 'nearest' else bool((a - b).abs().max() <= 1e-5 * b.abs().max())
            del ref
        seen_h = seen.cpu().numpy()
        nnz = int((idx >= 0).sum().item())
        moved = esz * m * F * (nnz + n_dst)                   # the rows read plus the rows written
        res = dict(method=method, k=k, n_src=n_src, n_dst=n_dst, features=F, m=m, dtype=args.dtype, bins=list(nb),
                   max_bin_occupancy=int(torch.bincount(key).max().item()), step_ms={s: stats(ms[s]) for s in STEPS},
                   inspected=dict(mean=float(seen_h.mean()), max=int(seen_h.max())), apply_bytes=moved,
                   apply_TBps=moved / (np.median(ms['apply']) * 1e-3) / 1e12,
                   torch_TBps=moved / (np.median(ms['torch']) * 1e-3) / 1e12,
                   apply_over_torch=float(np.median(ms['torch']) / np.median(ms['apply'])), torch_agrees=agree)
        if not args.no_scipy:
            from scipy.spatial import cKDTree
            t0 = time.perf_counter()
            tree = cKDTree(xyz)
            t1 = time.perf_counter()
            _, ref_idx = tree.query(grid.cell_centers(), k=k, workers=16)
            t2 = time.perf_counter()
            same = float(np.mean(ref_idx.reshape(n_dst, k) == idx.cpu().numpy()))
            res['ckdtree'] = dict(build_ms=(t1 - t0) * 1e3, query_ms=(t2 - t1) * 1e3, indices_equal=same)
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
