#!/usr/bin/env python3
"""Kernel micro-benchmark (GPU box): times each libspr_hip kernel with HIP events for a list of
shapes and prints ms, algorithmic GB/s and TFLOP/s.   python tools/kbench.py [cells,F,m,r ...]
python tools/kbench.py validate [--encode-only] [--host-route] [cells,F,r,k ...]: the held-out-snapshot kernels (encode,
field_error) next to reconstruct at the same shape in the same process, with their fraction of the one-read bound
(8 r + 8 k + 8) n bytes at 6.3 TB/s.
python tools/kbench.py field_std [cells,F,r,k,q ...]: the uncertainty-map kernels (field_std, diagonal and factor form; q = 0
skips the factor form) next to reconstruct at the same shape, alternating in the same process, with reconstruct's run-to-run
spread; the factor form also as 2 n r q k / time in TFLOP/s.
python tools/kbench.py design [cells,F,r ...]: the design sweep (csrc/design.hip; criterion A, with and without the score map)
next to the factor form of field_std with k = 1, q = r at the same shape -- the same bytes and the same product --,
alternating in the same process: ms, 2 n r^2 / time in TFLOP/s, the ratio and the factor form's run-to-run spread."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from openmeasure_amd.engine import HipEngine
from openmeasure_amd.synth import make_R


def timeit(fn, reps=5):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


HBM_ACHIEVABLE = 6.3e12     # bytes/s a streaming kernel reaches on this part (LAB_NOTEBOOK)


def validate(args):
    """encode / field_error against reconstruct: same basis, same k vectors, same process"""
    import time
    flags = {a for a in args if a.startswith('--')}
    shapes = [tuple(int(v) for v in a.split(',')) for a in args if not a.startswith('--')] or [(1_000_000, 4, 32, 16)]
    eng = HipEngine()
    held = None
    for cells, F, r, k in shapes:
        n = cells * F
        if held is None or held[0] != (n, r):
            held = None
            torch.cuda.empty_cache()
            g = torch.Generator(device=eng.device).manual_seed(1)
            Ur = torch.randn((n, r), generator=g, device=eng.device, dtype=torch.float64) / r ** 0.5
            mu = torch.randn((n,), generator=g, device=eng.device, dtype=torch.float64)
            held = ((n, r), Ur, mu)
        _, Ur, mu = held
        sc = eng.to_device(np.linspace(0.5, 2.0, F))
        A = eng.to_device(np.random.default_rng(0).standard_normal((k, r)))
        out = eng.reconstruct(Ur, 0, cells, F, mu, sc, A)                       # (k, n)
        Xt = (out.t() + 0.01).contiguous()                                       # (n, k) row-major, the layout of X
        bound = (8 * r + 8 * k + 8) * n
        t_e = timeit(lambda: eng.encode(Ur, 0, cells, F, mu, sc, Xt))
        print(f'rows={n} F={F} r={r} k={k}  basis {n * r * 8 / 1e9:.2f} GB  one-read bound {bound / 1e9:.2f} GB')
        print(f'  encode      {t_e:8.3f} ms  {bound / t_e / 1e6:8.1f} GB/s  {100 * bound / HBM_ACHIEVABLE / (t_e / 1e3):5.1f} % of bound  {2.0 * n * r * k / t_e / 1e9:7.2f} TF')
        if '--encode-only' in flags:
            del out, Xt
            continue
        t_r = timeit(lambda: eng.reconstruct(Ur, 0, cells, F, mu, sc, A, out=out))
        t_f = timeit(lambda: eng.field_error(Ur, 0, cells, F, mu, sc, A, Xt))
        print(f'  reconstruct {t_r:8.3f} ms  {bound / t_r / 1e6:8.1f} GB/s  (writes its {n * k * 8 / 1e9:.2f} GB field, reads no X_true)')
        print(f'  field_error {t_f:8.3f} ms  {bound / t_f / 1e6:8.1f} GB/s  {100 * bound / HBM_ACHIEVABLE / (t_f / 1e3):5.1f} % of bound   field_error / reconstruct = {t_f / t_r:.2f}')
        if '--host-route' in flags:
            # what reconstruction_error replaces: the field to the host, NumPy norms there
            xt_h = eng.to_host(Xt)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            field = eng.to_host(eng.reconstruct(Ur, 0, cells, F, mu, sc, A, out=out), result=True).T
            d = field - xt_h
            stats = [((d[f * cells:(f + 1) * cells] ** 2).sum(axis=0), np.abs(d[f * cells:(f + 1) * cells]).max(axis=0)) for f in range(F)]
            t_h = time.perf_counter() - t0
            t0 = time.perf_counter()
            rec = eng.to_host(eng.field_error(Ur, 0, cells, F, mu, sc, A, Xt))
            t_d = time.perf_counter() - t0
            assert np.allclose(rec[:, :, 0].T, np.stack([s_[0] for s_ in stats]), rtol=1e-9)
            print(f'  host route (reconstruct -> host -> NumPy) {1e3 * t_h:9.2f} ms   field_error + download of the records {1e3 * t_d:7.3f} ms   x{t_h / t_d:.0f}')
            del xt_h, field, d
        del out, Xt
        torch.cuda.empty_cache()


def field_std(args):
    """diagonal / factor form of field_std against reconstruct: same basis, same k, alternating in one process"""
    shapes = [tuple(int(v) for v in a.split(',')) for a in args] or [(1_000_000, 4, 64, 16, 64)]
    eng = HipEngine()
    held = None
    for cells, F, r, k, q in shapes:
        n = cells * F
        if held is None or held[0] != (n, r):
            held = None
            torch.cuda.empty_cache()
            g = torch.Generator(device=eng.device).manual_seed(1)
            Ur = torch.randn((n, r), generator=g, device=eng.device, dtype=torch.float64) / r ** 0.5
            mu = torch.randn((n,), generator=g, device=eng.device, dtype=torch.float64)
            held = ((n, r), Ur, mu)
        _, Ur, mu = held
        rng = np.random.default_rng(0)
        sc = eng.to_device(np.linspace(0.5, 2.0, F))
        A = eng.to_device(rng.standard_normal((k, r)))
        out = eng.empty((k, n))
        rec = lambda: eng.reconstruct(Ur, 0, cells, F, mu, sc, A, out=out)
        dia = lambda: eng.field_std(Ur, 0, cells, F, sc, S=A, out=out)
        t_r, t_d = [], []
        for _ in range(3):                                    # alternate: both see the same neighbours on the machine
            t_r.append(timeit(rec, reps=3))
            t_d.append(timeit(dia, reps=3))
        mr, md = float(np.median(t_r)), float(np.median(t_d))
        spread = (max(t_r) - min(t_r)) / mr
        nbytes = (8 * r + 8 * k) * n
        print(f'rows={n} F={F} r={r} k={k}  basis {n * r * 8 / 1e9:.2f} GB  written {n * k * 8 / 1e9:.2f} GB')
        print(f'  reconstruct    {mr:9.3f} ms  {(nbytes + 8 * n) / mr / 1e6:8.1f} GB/s  runs {" ".join(f"{t:.3f}" for t in t_r)}  spread {100 * spread:.1f} %')
        print(f'  field_std diag {md:9.3f} ms  {nbytes / md / 1e6:8.1f} GB/s  runs {" ".join(f"{t:.3f}" for t in t_d)}  diag / reconstruct = {md / mr:.3f}  (allowed {1 + max(0.10, 3 * spread):.3f})')
        if q > 0:
            L = eng.to_device(rng.standard_normal((k, r, q)) / q ** 0.5)
            t_f = timeit(lambda: eng.field_std(Ur, 0, cells, F, sc, L=L, out=out), reps=3)
            print(f'  field_std factor q={q} {t_f:9.3f} ms  {2.0 * n * r * q * k / t_f / 1e9:7.2f} TFLOP/s  {nbytes / t_f / 1e6:8.1f} GB/s')
        del out
        torch.cuda.empty_cache()


def design(args):
    """design sweep against the factor form of field_std (k = 1, q = r): same basis, same product, alternating"""
    shapes = [tuple(int(v) for v in a.split(',')) for a in args] or [(1_000_000, 4, 32), (1_000_000, 4, 64), (1_000_000, 4, 128)]
    eng = HipEngine()
    held = None
    for cells, F, r in shapes:
        n = cells * F
        if held is None or held[0] != (n, r):
            held = None
            torch.cuda.empty_cache()
            g = torch.Generator(device=eng.device).manual_seed(1)
            Ur = torch.randn((n, r), generator=g, device=eng.device, dtype=torch.float64) / r ** 0.5
            held = ((n, r), Ur)
        _, Ur = held
        rng = np.random.default_rng(0)
        A = rng.standard_normal((r, r))
        B = eng.to_device(A @ A.T / r + 0.1 * np.eye(r))
        sc = eng.to_device(np.linspace(0.5, 2.0, F))
        out = eng.empty((1, n))
        fac = lambda: eng.field_std(Ur, 0, cells, F, sc, L=B[None], out=out)
        swp = lambda: eng.design_sweep(Ur, 0, cells, F, B, sc, None, 'A')
        swm = lambda: eng.design_sweep(Ur, 0, cells, F, B, sc, None, 'A', scores=out[0])
        t_f, t_s, t_m = [], [], []
        for _ in range(3):                                    # alternate: all see the same neighbours on the machine
            t_f.append(timeit(fac, reps=3))
            t_s.append(timeit(swp, reps=3))
            t_m.append(timeit(swm, reps=3))
        mf, ms, mm = (float(np.median(t)) for t in (t_f, t_s, t_m))
        spread = (max(t_f) - min(t_f)) / mf
        flops = 2.0 * n * r * r
        print(f'rows={n} F={F} r={r}  basis {n * r * 8 / 1e9:.2f} GB')
        print(f'  field_std factor k=1 q=r {mf:9.3f} ms  {flops / mf / 1e9:7.2f} TFLOP/s  {8.0 * n * r / mf / 1e6:8.1f} GB/s  runs {" ".join(f"{t:.3f}" for t in t_f)}  spread {100 * spread:.1f} %')
        print(f'  design sweep (no map)    {ms:9.3f} ms  {flops / ms / 1e9:7.2f} TFLOP/s  {8.0 * n * r / ms / 1e6:8.1f} GB/s  runs {" ".join(f"{t:.3f}" for t in t_s)}  sweep / factor = {ms / mf:.3f}')
        print(f'  design sweep (+ map)     {mm:9.3f} ms  {flops / mm / 1e9:7.2f} TFLOP/s  runs {" ".join(f"{t:.3f}" for t in t_m)}  sweep / factor = {mm / mf:.3f}')
        del out
        torch.cuda.empty_cache()


def main():
    if sys.argv[1:2] == ['design']:
        return design(sys.argv[2:])
    if sys.argv[1:2] == ['validate']:
        return validate(sys.argv[2:])
    if sys.argv[1:2] == ['field_std']:
        return field_std(sys.argv[2:])
    shapes = [tuple(int(v) for v in a.split(',')) for a in sys.argv[1:]] or [(1_000_000, 4, 64, 32), (1_000_000, 9, 256, 64)]
    eng = HipEngine()
    lib = eng.lib
    for cells, F, m, r in shapes:
        n = cells * F
        R = eng.to_device(make_R(m, r))
        X = eng.synth(n, m, 0, cells, R, 1e-3, 1)
        rowmean = eng.empty((n,)); fstats = eng.empty((F, 3)); gram = eng.empty((F, m, m))
        ws = eng._workspace('gram', lib.spr_stats_gram_workspace(m, F))
        st = eng._stream()
        t_g = timeit(lambda: lib.spr_stats_gram_f64(X.data_ptr(), n, m, m, 0, cells, F, 1, rowmean.data_ptr(), ws.data_ptr(), ws.numel(), st))
        t_f = timeit(lambda: lib.spr_stats_gram_finalize_f64(n, m, 0, cells, F, ws.data_ptr(), ws.numel(), fstats.data_ptr(), gram.data_ptr(), m, 0, st))
        W = eng.to_device(np.random.default_rng(0).standard_normal((m, r)))
        inv = eng.to_device(np.ones(F))
        Ur = eng.project(X, 0, cells, F, inv, W, rowmean=rowmean)
        t_p = timeit(lambda: eng.project(X, 0, cells, F, inv, W, out=Ur, rowmean=rowmean))
        a = eng.to_device(np.ones((1, r))); out = eng.empty((1, n))
        t_r = timeit(lambda: eng.reconstruct(Ur, 0, cells, F, rowmean, inv, a, out=out))
        qs = eng.qr_begin(Ur, 0, 8)
        eng.qr_step(qs, 0, qs['rec'][None], qs['tau'][None], True)
        t_q = timeit(lambda: eng.qr_refresh(qs, 0, 1))
        for j in range(1, 8):
            eng.qr_step(qs, j, qs['rec'][None], qs['tau'][None], True)
        t_q8 = timeit(lambda: eng.qr_refresh(qs, 0, 8))
        t_n = timeit(lambda: eng.qr_begin(Ur, 0, 8))
        xb = n * m * 8
        print(f'cells={cells} F={F} m={m} r={r}  X={xb / 1e9:.2f} GB')
        print(f'  stats_gram  {t_g:8.3f} ms  {xb / t_g / 1e6:8.1f} GB/s  {n * m * m / t_g / 1e9:7.2f} TF   (finalize {t_f:.3f} ms)')
        print(f'  project     {t_p:8.3f} ms  {(xb + n * r * 8) / t_p / 1e6:8.1f} GB/s  {2.0 * n * m * r / t_p / 1e9:7.2f} TF')
        print(f'  reconstruct {t_r:8.3f} ms  {(n * r * 8 + 16 * n) / t_r / 1e6:8.1f} GB/s')
        print(f'  qr_sweep x1 {t_q:8.3f} ms  {(n * r * 8 + 16 * n) / t_q / 1e6:8.1f} GB/s   x8 directions {t_q8:8.3f} ms  {(n * r * 8 + 16 * n) / t_q8 / 1e6:8.1f} GB/s   init(norms+cands) {t_n:8.3f} ms')
        del X, Ur, out, rowmean
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
