#!/usr/bin/env python3
"""Time one camera.project(to_host=False) at the scale of the reference's notebook: 64^3 cells, a 512^2 sensor, the parallel
model and the pinhole model with N_rand = 4.  Warm-up 2, 7 repetitions; per kernel the median with min - max from stream
events, the entry counts, and the bytes of the traffic model (16 B per entry, written and read once per stage).

    python tools/raycast_probe.py [--cells 64] [--sensor 512] [--reps 7] [--warmup 2] [--grid voxel|rect|both]

--grid voxel casts the VoxelGrid through the uniform kernels; rect casts RectilinearGrid.from_voxel_grid of it -- the same
cells -- through the rectilinear kernels (stored edges, bisection); both alternates the two within every repetition, so
that their difference is not a difference between two processes, and reports whether they gave the same matrix.

Prints one JSON line per model and grid."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNELS = ('raycast_count', 'raycast_fill', 'raycast_merge', 'raycast_compact')


def stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cells', type=int, default=64)
    ap.add_argument('--sensor', type=int, default=512)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--grid', choices=('voxel', 'rect', 'both'), default='voxel')
    args = ap.parse_args()
    import torch
    from openmeasure_amd.engine import HipEngine
    from openmeasure_amd.utils import VoxelGrid, camera

    eng = HipEngine('cuda:0')
    n, px = args.cells, args.sensor
    voxel = VoxelGrid((-0.2, -0.2, 0.1), (0.4 / n,) * 3, (n, n, n))         # the sensor's 0.4 x 0.4 field of view, 0.4 deep
    grids = {}
    if args.grid in ('voxel', 'both'):
        grids['voxel'] = voxel
    if args.grid in ('rect', 'both'):
        from openmeasure_amd.utils import RectilinearGrid
        grids['rect'] = RectilinearGrid.from_voxel_grid(voxel)
    cam = camera(np.array([1., 0., 0.3, 1]), np.array([-np.pi / 2, 0., -np.pi / 2]), 1, 1, 1, np.array([px, px]), 0.4 / px)
    for type_rec, n_rand in (('parallel', 1), ('pinhole', 4)):
        a, b = cam.segments(type_rec, n_rand, seed=0)
        seg = np.concatenate([a, b], axis=2).reshape(-1, 6)
        n_ray = a.shape[1]
        ms = {g: {k: [] for k in KERNELS} for g in grids}
        wall, host, out = {g: [] for g in grids}, [], {}
        for rep in range(args.warmup + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a, b = cam.segments(type_rec, n_rand, seed=0)
            if rep >= args.warmup:
                host.append((time.perf_counter() - t0) * 1e3)
            for g, grid in grids.items():
                t1 = time.perf_counter()
                ev = {k: eng.time_next(k) for k in KERNELS}
                out[g] = eng.raycast(seg, grid, n_ray, 'hit', 0)
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                if rep >= args.warmup:
                    for k in KERNELS:
                        ms[g][k].append(eng.elapsed_ms(*ev[k]))
                    wall[g].append((t2 - t1) * 1e3)
        # the same cells up to the rounding of origin + k * spacing (NumPy's edges against the kernel's fma): the same matrix
        same = all(torch.equal(x, y) for x, y in zip(out['voxel'], out['rect'])) if len(out) == 2 else None
        for g, grid in grids.items():
            raw = int(eng.raycast_count(eng.to_device(seg), grid).sum().item())
            nnz = int(out[g][1].shape[0])
            # count reads the segments; fill writes the raw entries; merge reads them and writes the fronts; compact reads
            # the fronts and writes the matrix
            model = dict(raycast_count=seg.nbytes + 8 * seg.shape[0], raycast_fill=seg.nbytes + 16 * raw,
                         raycast_merge=16 * raw + 16 * nnz, raycast_compact=16 * nnz + 16 * nnz)
            print(json.dumps(dict(model=type_rec, grid=g, cells=n ** 3, pixels=px * px, n_ray=n_ray, segments=int(seg.shape[0]),
                                  raw_entries=raw, nnz=nnz, same_matrix=same, kernel_ms={k: stats(ms[g][k]) for k in KERNELS},
                                  model_bytes=model, raycast_wall_ms=stats(wall[g]), segments_host_ms=stats(host))), flush=True)

if __name__ == '__main__':
    main()
