"""The double-buffered panel sweep that the four vector-stationary basis kernels each carry (reconstruct_mfma_kernel,
bound_sweep_mfma_kernel, field_error_mfma_kernel, field_std_diag_kernel): eng.reconstruct, eng.bound_sweep,
eng.field_error and eng.field_std(S=...) on every rung of the padded width,
in every load mode, with f64 and f32 basis storage, at shapes where the double-buffered pipeline turns over.

Shapes.  One r per rung (16 MTR columns, MTR = 1, 2, 3, 4, 6, 8) and load mode: r = 16 MTR with packed rows (mode 2: pairs, no
column tail), an even r below it in rows of even length (mode 1: pairs with a column tail), an odd r (mode 0: scalar loads).
Three features of n_points rows, n_points = 64 * 3 w + 37 with w the workgroups the launchers deal to a feature (per-CU
table of launch.hpp x spr_device_cus, a third each): every feature has 3 w + 1 panels, so every workgroup takes at least
three -- first, next and after-next panel are all staged -- under the strided deal as under bound_sweep's contiguous runs,
and every feature ends in a panel of 37 rows (two full 16-row blocks of a wave, one of 5 rows, one empty).  k = 17 vectors:
a second pass with a single vector.  One more case per kernel on a window that starts inside feature 0 and ends inside
feature 2.

References and bars are those of the kernels' own test files, imported from them:
 * reconstruct: tests/test_validate_host.numpy_field_error against a zero field is the reconstruction and its per-entry
   rounding bound delta = (r + 6) 2^-53 (|X_cnt| + X_scl sum |Ur a|); two computed values, each within delta of the exact
   one: 2 delta, entry by entry (as test_validate_host.check_errors compares f64 with f64);
 * field_error: tests/test_validate_gpu._check_field_error, in the form it gives a long block (f64 products, longdouble
   sums, the bar tightened by the reference's own error, max_row exact);
 * field_std: tests/test_field_std_gpu._run / _check: a sample of rows in longdouble at the bar, all rows at twice the bar
   against the f64 form (tests/test_field_std_gpu.test_long_block_both_forms);
 * bound_sweep: tests/test_cols_host.scaled_limits and _feas_round (rnd: two summation orders of one dot product), as
   tests/test_cols_gpu uses them.  Beyond the maxima and counts checked there, the candidates are held to the contiguous
   runs of panels the launcher deals: at most one candidate per (run, side), each the worst row of its run, none missing.
   Where the run's leader leads by more than rnd -- asserted for every reported candidate -- that names the row exactly."""
import numpy as np
import pytest

from tests.test_cols_host import _feas_round, scaled_limits
from tests.test_field_std_gpu import _check as check_field_std, _run as run_field_std
from tests.test_field_std_host import variance_bar_diag
from tests.test_validate_gpu import _check_field_error
from tests.test_validate_host import numpy_field_error

pytestmark = pytest.mark.gpu
F, K = 3, 17
PER_CU = {1: 6, 2: 4, 3: 3, 4: 2, 6: 1, 8: 1}                 # workgroups per CU by LDS: spr_panel_per_cu of launch.hpp
# (r, padding of the row): mode 2, mode 1, mode 0 of each rung
R_PAD = [(16, 0), (32, 0), (48, 0), (64, 0), (96, 0), (128, 0),
         (6, 2), (24, 2), (40, 2), (56, 2), (80, 2), (112, 2),
         (5, 0), (17, 0), (33, 0), (49, 0), (65, 0), (97, 0)]


@pytest.fixture(scope='module')
def eng():
    from openmeasure_amd.engine import HipEngine
    return HipEngine('cuda:0')


def _rung(r):
    return next(mt for mt in (1, 2, 3, 4, 6, 8) if r <= 16 * mt)


def _total_wg(eng, r):
    import ctypes
    cus = ctypes.c_int(0)
    assert eng.lib.spr_device_cus(ctypes.byref(cus)) == 0 and cus.value > 0
    return PER_CU[_rung(r)] * cus.value


def _seg_wgs(rows, n, total_wg):
    """workgroups of a feature segment of `rows` rows in a block of n (common.hpp, 64-row panels)"""
    return max(1, min(rows * total_wg // n, -(-rows // 64)))


def _runs(row0, n, n_points, total_wg):
    """first local row of every workgroup's contiguous run of panels (bounds.hip, panel_run), in block order; the runs
    tile [0, n)"""
    starts = []
    for f in range(row0 // n_points, min((row0 + n - 1) // n_points, F - 1) + 1):
        lo, hi = max(f * n_points, row0) - row0, min((f + 1) * n_points, row0 + n) - row0
        npanels = -(-(hi - lo) // 64)
        w = _seg_wgs(hi - lo, n, total_wg)
        starts += [lo + 64 * (npanels * wl // w) for wl in range(w)]
    assert starts[0] == 0 and np.all(np.diff(starts) >= 64)
    return np.array(starts)


def _case(eng, r, pad, f32, window=False):
    import torch
    total = _total_wg(eng, r)
    w = total // F
    n_points = 64 * 3 * w + 37
    row0, n = (n_points // 2 + 5, 2 * n_points) if window else (0, F * n_points)
    if not window:                                             # every workgroup of every feature: at least three panels
        assert _seg_wgs(n_points, n, total) == w and (3 * w + 1) // w >= 3
    rng = np.random.default_rng(9000 + 10 * r + f32)
    U = rng.standard_normal((n, r)) / np.sqrt(r)
    if f32:
        U = U.astype(np.float32)
    buf = np.zeros((n, r + pad), dtype=U.dtype)
    buf[:, :r] = U
    Ud = eng.to_device(buf, dtype=torch.float32 if f32 else torch.float64)[:, :r]
    assert Ud.stride(0) == r + pad
    mu = rng.standard_normal(n) * 0.3
    scale = rng.uniform(0.5, 2.0, F)
    A = rng.standard_normal((K, r))
    return dict(Ud=Ud, U=U.astype(np.float64), mu=mu, scale=scale, A=A, row0=row0, n=n, n_points=n_points, F=F, r=r, k=K,
                long=True, total_wg=total, rng=rng)


def _check_reconstruct(eng, c, tag):
    out = eng.to_host(eng.reconstruct(c['Ud'], c['row0'], c['n_points'], F, eng.to_device(c['mu']),
                                      eng.to_device(c['scale']), eng.to_device(c['A'])))
    assert out.shape == (K, c['n'])
    ref = numpy_field_error(c['U'], c['row0'], c['n_points'], F, c['mu'], c['scale'], c['A'], np.zeros((c['n'], K)))
    err = np.abs(out.T - ref['d'])
    print('reconstruct', tag, 'worst error / bar', (err / (2 * ref['delta'])).max())
    assert np.all(err <= 2 * ref['delta']), tag


def _check_field_std(eng, c, tag):
    S = c['rng'].standard_normal((K, c['r']))
    n, row0, n_points = c['n'], c['row0'], c['n_points']
    out = run_field_std(eng, c['Ud'], row0, n_points, F, c['scale'], S=S)
    s = c['scale'][np.minimum((row0 + np.arange(n)) // n_points, F - 1)]
    cuts = [g * n_points - row0 for g in range(1, F) if 0 < g * n_points - row0 < n]
    rows = np.unique(np.clip(np.concatenate([np.arange(256), n - 1 - np.arange(256)] + [q + np.arange(-130, 130) for q in cuts]
                                            + [c['rng'].integers(0, n, 1000)]), 0, n - 1))
    check_field_std(out, c['U'], None, s, tag, rows=rows, S=S)
    want, bar = variance_bar_diag(c['U'], S, s)
    assert np.all(np.abs(out ** 2 - want) <= 2 * bar), tag


def _check_field_error_case(eng, c, tag):
    import torch
    feat = np.minimum((c['row0'] + np.arange(c['n'])) // c['n_points'], F - 1)
    # a field near the reconstruction, as tests/test_validate_gpu._case makes it
    X = (c['U'] @ c['A'].T) * c['scale'][feat][:, None] + c['mu'][:, None] + 0.05 * c['rng'].standard_normal((c['n'], K))
    _check_field_error(eng, dict(c, X=X, Xd=eng.to_device(X, dtype=torch.float64)), tag)


def _check_bound_sweep(eng, c, tag):
    rng, U, row0, n, n_points = c['rng'], c['U'], c['row0'], c['n'], c['n_points']
    G = c['A']
    limits = np.stack([-rng.uniform(1.0, 2.5, F), rng.uniform(1.0, 2.5, F)])
    clamp = np.full((2, F), np.nan)
    lo0, hi0, _ = scaled_limits(row0, n, n_points, F, c['mu'], c['scale'], limits, clamp)
    x = U @ G.T
    v2 = np.stack([lo0[:, None] - x, x - hi0[:, None]], axis=2)          # (n, K, side)
    starts = _runs(row0, n, n_points, c['total_wg'])
    run_of = np.repeat(np.arange(len(starts)), np.diff(np.append(starts, n)))
    runmax = np.maximum.reduceat(v2, starts, axis=0)                     # (runs, K, side)
    rnds = _feas_round(U, np.ones(1)) * np.linalg.norm(G, axis=1)        # 2 r eps max |u|_2 |g|_2 per vector
    vmax = v2.max(axis=2)                                                # (n, K): the violation of a row
    args = (c['Ud'], row0, n_points, F, eng.to_device(c['mu']), eng.to_device(c['scale']), eng.to_device(limits),
            eng.to_device(clamp), eng.to_device(G))
    # tol 0.05: thousands of runs violate, the k candidates are the worst of them; the second tol leaves vector 0 ten
    # violating (run, side) pairs (fewer where not even ten violate at tol = 0), fewer than k: every one of them is reported
    top = np.sort(runmax[:, 0, :].ravel())[::-1]
    for tol, k in ((0.05, 24), (max(0.5 * (top[9] + top[10]), 0.0), 24)):
        out = eng.to_host(eng.bound_sweep(*args, tol, k))
        assert out.shape == (K, 3 + 3 * k)
        sures, maybes = (vmax > tol + rnds).sum(axis=0), (vmax > tol - rnds).sum(axis=0)
        for p in range(K):
            rnd, v = rnds[p], vmax[:, p]
            assert abs(out[p, 0] - v.max()) <= rnd
            row = int(out[p, 1]) - row0
            assert 0 <= row < n and v[row] >= v.max() - rnd
            assert sures[p] <= int(out[p, 2]) <= maybes[p], (tag, p, sures[p], int(out[p, 2]), maybes[p])
            cand = out[p, 3:].reshape(k, 3)
            used = cand[cand[:, 0] >= 0]
            assert np.all(cand[len(used):, 0] == -1) and np.all(np.isneginf(cand[len(used):, 2]))
            rm = runmax[:, p, :]
            assert min(k, np.count_nonzero(rm > tol + rnd)) <= len(used) <= min(k, np.count_nonzero(rm > tol - rnd))
            if len(used) == 0:
                continue
            assert int(used[0, 0]) == int(out[p, 1]) and used[0, 2] == out[p, 0]      # the global worst is the first candidate
            assert np.all(np.diff(used[:, 2]) <= 0)                                  # worst first
            rows, sides, vals = used[:, 0].astype(np.int64) - row0, used[:, 1].astype(np.int64), used[:, 2]
            assert np.all((rows >= 0) & (rows < n)) and np.all((sides == 0) | (sides == 1)) and np.all(vals > tol)
            runs = run_of[rows]
            assert len(set(zip(runs.tolist(), sides.tolist()))) == len(used)         # one candidate per (run, side)
            assert np.all(np.abs(v2[rows, p, sides] - vals) <= rnd)
            # the worst row of its run: the leader leads by more than rnd (precondition), and it is the row reported
            for rw, sd, ru in zip(rows, sides, runs):
                seg = v2[starts[ru]:(starts[ru + 1] if ru + 1 < len(starts) else n), p, sd]
                lead = np.partition(seg, -2)[-2:]
                assert lead[1] - lead[0] > rnd, (tag, p, 'no exact worst row')
                assert rw == starts[ru] + int(np.argmax(seg)), (tag, p, int(rw))
            # none missing: whatever was left out is no worse than the last one reported (k of them) or than tol
            left = np.ones(rm.shape, dtype=bool)
            left[runs, sides] = False
            floor = vals[-1] if len(used) == k else tol
            assert np.all(rm[left] <= floor + rnd), (tag, p)


CASES = [(r, pad, f32) for r, pad in R_PAD for f32 in (False, True)]


@pytest.mark.parametrize('r,pad,f32', CASES, ids=[f'r{r}-{"u32" if f32 else "u64"}' for r, pad, f32 in CASES])
def test_four_entries_every_rung_load_mode_and_storage(eng, r, pad, f32):
    c = _case(eng, r, pad, f32)
    tag = (r, pad, f32)
    _check_reconstruct(eng, c, tag)
    _check_bound_sweep(eng, c, tag)
    _check_field_error_case(eng, c, tag)
    _check_field_std(eng, c, tag)


def test_four_entries_on_a_row_window(eng):
    """rows [n_points / 2 + 5, + 2 n_points): starts inside feature 0, ends inside feature 2; r = 40 (MTR 3, pairs)"""
    c = _case(eng, 40, 2, False, window=True)
    assert c['row0'] != 0 and c['row0'] % c['n_points'] and (c['row0'] + c['n']) % c['n_points']
    tag = ('window', 40)
    _check_reconstruct(eng, c, tag)
    _check_bound_sweep(eng, c, tag)
    _check_field_error_case(eng, c, tag)
    _check_field_std(eng, c, tag)
