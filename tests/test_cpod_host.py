"""ROM.CPOD({'limits': [lo, hi]}) (openmeasure_amd/_cpod.py) on the CPU: the constraint-generation loop and the working-set
solve, with the NumPy bound sweep of tests/test_cols_host.py (ColsNumpyEngine has no bound_sweep_batch, so the driver's
fallback to bound_sweep is what runs here; the HIP kernels are held to the same bars in tests/test_cpod_gpu.py).

Yardsticks (cvxpy is not installed, the reference cannot run this method): per snapshot i, with a = Ar0[i] the coefficients
fit() left, (lo0, hi0) = scale_limits(limits), g = the returned row and lambda the returned multipliers,
 (i)  the KKT conditions of the FULL problem  min 1/2 |g - a|^2, lo0 <= Ur g <= hi0  in NumPy f64: feasibility over all n
      rows <= cpod_tol + _feas_round(U, g), lambda >= 0, stationarity |g - a + A^T lambda|_inf / |a|_inf, complementarity
      |lambda (A g - b)|_inf / lambda_max.  The problem is strictly convex: a point that meets them is the solution;
 (ii) SciPy's SLSQP on the full 2 n constraints, started from a, counted only where it reports success and its own point is
      feasible to 1e-9.

Measured on this loop (own Lawson-Hanson solve + NumPy sweep) over the three cases CASES (seed, n_points, F, m, r):
    (1, 400, 2, 24, 6)    24/24 violate at the start   7 rounds  27 rows   stationarity 2.3e-17 ... 1.6e-16   compl. 2.2e-18 ... 1.8e-16
    (2, 300, 3, 32, 10)   32/32                        8 rounds  41 rows                2.6e-17 ... 1.6e-16           6.5e-19 ... 2.5e-16
    (3, 1000, 2, 40, 16)  40/40                        7 rounds  58 rows                2.1e-17 ... 1.3e-16           1.1e-18 ... 3.1e-16
    |g - g_SLSQP|_inf / |g|_inf where SLSQP counts (first four snapshots of each case; all twelve counted): 2.8e-16 ... 4.1e-14
Bars = 10 x the worst measured figure (the margin is for another summation order in the MFMA sweep), the rule
tests/test_cols_host.py documents:
    STAT_BAR = 1.7e-15      COMP_BAR = 3.1e-15      SLSQP_BAR = 4.2e-13

Two correct runs that generate DIFFERENT working sets (sharded against single-process, batched sweep against the 16-vector
sweep: other workgroup runs, other candidates) are compared with SAME_BAR.  Both points g1, g2 are projections of a onto
polytopes that contain the feasible set K, so |g_i - a| <= |g* - a| for the solution g*, and both lie within cpod_tol of
every constraint; for the projection onto a convex set, |g_i - g*|^2 <= |g_i' - a|^2 - |g* - a|^2 for any g_i' in K, and
with g_i' a point of K at distance delta from g_i this is <= 2 |g* - a| delta + delta^2.  delta is cpod_tol times a
geometry constant taken as 1 / min |u_row| over the working rows (moving along a row's own direction); SAME_BAR is evaluated
per comparison from these quantities (same_bar below), about 2e-2 absolute here -- a loose bound by construction;
the figures measured are printed next to it.  It is NOT what certifies the second run: each of the two results is held to
(i) on the full problem by itself -- the sharded one in the parent process, from the ranks' own blocks of Ur, their scaled
limits and their multipliers (kkt_check), so a binding row the other rank missed fails feasibility there.
"""
import os
import pickle
import sys

import numpy as np
import pytest

from openmeasure_amd.sparse_sensing import ROM, SPR
from tests.numpy_engine import NumpyEngine
from tests.test_cols_host import ColsNumpyEngine, _feas_round, _free_port, make_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
STAT_BAR, COMP_BAR = 1.7e-15, 3.1e-15
SLSQP_BAR = 4.2e-13
CASES = {'c1': dict(seed=1, n_points=400, F=2, m=24, r=6), 'c2': dict(seed=2, n_points=300, F=3, m=32, r=10),
         'c3': dict(seed=3, n_points=1000, F=2, m=40, r=16)}


def fitted(case, engine=None, cls=ROM, **knobs):
    rom = cls(case['X'], case['F'], None, engine=engine or ColsNumpyEngine())
    rom.fit(select_modes='number', n_modes=case['r'])
    for k, v in knobs.items():
        setattr(rom, k, v)
    return rom


def same_bar(rom, Ar0):
    """|g1 - g2|_2 bound for two correct CPOD results with different working sets (module docstring)"""
    U = np.asarray(rom.Ur, dtype=np.float64)
    rows = np.unique(np.concatenate([np.asarray(r) for r in rom.cpod_info_['rows']] + [np.zeros(0, dtype=np.int64)]))
    umin = np.sqrt((U[rows] ** 2).sum(axis=1)).min() if len(rows) else 1.0
    delta = rom.cpod_tol / umin
    dist = np.sqrt(((rom.Ar - Ar0) ** 2).sum(axis=1)).max()
    return 2 * np.sqrt(2 * dist * delta + delta * delta)


def kkt_all(rom, Ar0, limits, report=None, tag='CPOD'):
    """asserts (i) for every snapshot of a finished CPOD call; -> list of per-snapshot figures"""
    lo0, hi0 = rom.scale_limits(limits)
    return kkt_check(np.asarray(rom.Ur, dtype=np.float64), lo0, hi0, rom.cpod_tol, rom.Ar, Ar0, rom.cpod_info_, report, tag)


def kkt_check(U, lo0, hi0, cpod_tol, Ar, Ar0, info, report=None, tag='CPOD'):
    """(i) from plain arrays: U (n, r) the WHOLE basis, lo0 / hi0 (n,) the scaled limits of all rows, Ar the returned and
    Ar0 the fit's coefficients, info the per-snapshot lists of cpod_info_ (rows are global row numbers)"""
    out = []
    assert 'infeasible' not in info['status']
    for p in range(Ar0.shape[0]):
        g, a = Ar[p], Ar0[p]
        rows, sides, lam = info['rows'][p], info['sides'][p], info['multipliers'][p]
        assert info['status'][p] in ('ols', 'optimal') and info['max_violation'][p] <= cpod_tol
        x = U @ g
        viol = max((x - hi0).max(), (lo0 - x).max())
        assert viol <= cpod_tol + _feas_round(U, g), (p, viol)
        assert len(rows) == len(sides) == len(lam) and np.all(lam >= 0)
        sign = np.where(sides == 1, 1.0, -1.0)
        A = sign[:, None] * U[rows]
        b = np.where(sides == 1, hi0[rows], -lo0[rows])
        stat = np.abs(g - a + A.T @ lam).max() / np.abs(a).max()
        comp = np.abs(lam * (A @ g - b)).max() / max(lam.max(), 1e-300) if len(lam) else 0.0
        line = dict(p=p, status=info['status'][p], rounds=info['rounds'][p], rows=len(rows), viol=viol, stat=stat, comp=comp)
        print(tag, line)
        out.append(line)
        assert stat <= STAT_BAR and comp <= COMP_BAR, line
    if report is not None:
        report += out
    return out


def slsqp_full(U, a, lo0, hi0):
    from scipy.optimize import minimize
    s = 1.0 / max(a @ a, 1e-300)
    cons = [dict(type='ineq', fun=lambda g: hi0 - U @ g, jac=lambda g: -U),
            dict(type='ineq', fun=lambda g: U @ g - lo0, jac=lambda g: U)]
    res = minimize(lambda g: 0.5 * s * (g - a) @ (g - a), a, jac=lambda g: s * (g - a), constraints=cons, method='SLSQP',
                   options=dict(ftol=1e-15, maxiter=500))
    x = U @ res.x
    ok = bool(res.success) and max((x - hi0).max(), (lo0 - x).max()) <= 1e-9
    return res.x, ok


@pytest.mark.parametrize('name', sorted(CASES))
def test_cpod_against_kkt_and_slsqp(name):
    case = make_case(**CASES[name])
    rom = fitted(case)
    Ar0, S0 = np.array(rom.Ar), np.array(rom.Sigma_r)
    U = np.asarray(rom.Ur, dtype=np.float64)
    lo0, hi0 = rom.scale_limits(case['limits'])
    x0 = U @ Ar0.T
    start = np.maximum(x0 - hi0[:, None], lo0[:, None] - x0).max(axis=0)
    assert np.all(start > rom.cpod_tol)                       # every snapshot violates at the start: nothing is skipped
    assert rom.CPOD({'limits': case['limits']}, solver='CLARABEL', verbose=False, max_iter=100) is None
    info = rom.cpod_info_
    assert rom.Ar.shape == Ar0.shape and info['status'] == ['optimal'] * case['X'].shape[1]
    assert info['sweeps'] == max(info['rounds']) and min(info['rounds']) >= 2
    assert set(info) >= {'status', 'rounds', 'rows', 'sides', 'multipliers', 'max_violation', 'sweeps', 'sweep_seconds',
                         'qp_seconds'}
    np.testing.assert_array_equal(rom.Sigma_r, S0)
    np.testing.assert_array_equal(rom.Vr, rom.Ar / S0)
    assert 'X0' not in rom._host
    lines = kkt_all(rom, Ar0, case['limits'])
    print('CPOD', name, 'rounds', max(info['rounds']), 'rows', max(len(r) for r in info['rows']),
          'stat', max(l['stat'] for l in lines), 'comp', max(l['comp'] for l in lines))
    counted = 0
    for p in range(4):
        gs, ok = slsqp_full(U, Ar0[p], lo0, hi0)
        if ok:
            counted += 1
            d = np.abs(rom.Ar[p] - gs).max() / np.abs(rom.Ar[p]).max()
            print('CPOD slsqp', name, p, d)
            assert d <= SLSQP_BAR, (p, d)
    print('CPOD slsqp counted', name, counted)
    assert counted >= 1                                        # (measured: 4 of 4 in every case) the yardstick must not vanish
    # the reconstructed field respects the limits
    xr = rom.reconstruct(rom.Ar)
    n_pt = case['n_points']
    for f in range(case['F']):
        blk = xr[f * n_pt:(f + 1) * n_pt]
        delta = rom.cpod_tol * rom._scl_f[f] + 8 * EPS * max(abs(case['limits'][0][f]), abs(case['limits'][1][f]), 1.0) \
            + max(_feas_round(U, g) for g in rom.Ar) * rom._scl_f[f]
        assert blk.min() >= case['limits'][0][f] - delta and blk.max() <= case['limits'][1][f] + delta
    # a second call starts from the coefficients of the fit again
    first = rom.Ar.copy()
    rom.CPOD({'limits': case['limits']})
    np.testing.assert_array_equal(rom.Ar, first)
    np.testing.assert_array_equal(rom._cpod_Ar0, Ar0)


def test_non_binding_limits_leave_ar_bit_identical():
    case = make_case(**CASES['c1'])
    rom = fitted(case)
    Ar0, Vr0 = np.array(rom.Ar), np.array(rom.Vr)
    rom.CPOD({'limits': [case['limits'][0] - 50.0, case['limits'][1] + 50.0]})
    assert rom.cpod_info_['status'] == ['ols'] * case['X'].shape[1] and rom.cpod_info_['sweeps'] == 1
    np.testing.assert_array_equal(rom.Ar, Ar0)
    np.testing.assert_allclose(rom.Vr, Vr0, rtol=4 * EPS, atol=0)      # fit(): V / |V|; here: Ar / Sigma_r
    assert 'X0' not in rom._host


def test_clamped_feature():
    """(limit - X_cnt) / X_scl beyond +-1000 -> the constant replaces the scaled limit of the whole feature block (:201-204)"""
    case = make_case(seed=9, n_points=500, F=3, m=30, r=8, offset=3.0)
    rom = fitted(case)
    lim = [case['limits'][0].copy(), case['limits'][1].copy()]
    lim[1][1] += 5000.0 * rom._scl_f[1]
    lim[0][2] -= 5000.0 * rom._scl_f[2]
    lo0, hi0 = rom.scale_limits(lim)
    n_pt = case['n_points']
    assert np.all(hi0[n_pt:2 * n_pt] == 1000) and np.all(lo0[2 * n_pt:] == -1000)
    Ar0 = np.array(rom.Ar)
    rom.CPOD({'limits': lim})
    assert 'optimal' in rom.cpod_info_['status']
    kkt_all(rom, Ar0, lim)


def test_contradictory_limits_give_nan_rows():
    case = make_case(**CASES['c1'])
    rom = fitted(case)
    S0 = np.array(rom.Sigma_r)
    bad = [case['limits'][0].copy(), case['limits'][1].copy()]
    bad[0][1], bad[1][1] = bad[1][1], bad[0][1]                # lo > hi on feature 1
    rom.CPOD({'limits': bad})
    assert rom.cpod_info_['status'] == ['infeasible'] * case['X'].shape[1]
    assert np.all(np.isnan(rom.Ar)) and np.all(np.isnan(rom.Vr))
    np.testing.assert_array_equal(rom.Sigma_r, S0)
    rom.CPOD({'limits': case['limits']})                        # the centre is still the fit's: the object recovers
    assert rom.cpod_info_['status'] == ['optimal'] * case['X'].shape[1] and np.all(np.isfinite(rom.Ar))


def test_refusals():
    case = make_case(**CASES['c1'])
    lim = {'limits': case['limits']}
    rom = fitted(case)
    for pd in ({}, {'problem': object(), 'g': object(), 'x0': object()}, None):
        with pytest.raises(NotImplementedError):
            rom.CPOD(pd)
    with pytest.raises(ValueError, match='limits'):
        rom.CPOD({'limits': [case['limits'][0]]})
    # a basis fit() did not compute
    other = fitted(case)
    rom.fit(basis=(np.asarray(other.Ur), np.asarray(other.Ar)))
    with pytest.raises(NotImplementedError, match='basis='):
        rom.CPOD(lim)
    rom.fit(select_modes='number', n_modes=case['r'])
    rom.CPOD(lim)                                              # a fit of its own again: built path
    rom.Ur = np.asarray(rom.Ur).copy()
    with pytest.raises(NotImplementedError, match='assigned'):
        rom.CPOD(lim)
    spr = fitted(case, cls=SPR)
    mask = np.ones(case['X'].shape[0], dtype=bool)
    mask[:50] = False
    spr.optimal_placement(mask=mask)
    with pytest.raises(NotImplementedError, match='mask'):
        spr.CPOD(lim)
    plain = fitted(case, engine=NumpyEngine())                 # no bound_sweep: no CPU fallback
    with pytest.raises(NotImplementedError, match='bound sweep'):
        plain.CPOD(lim)
    unfit = ROM(case['X'], case['F'], None, engine=ColsNumpyEngine())
    with pytest.raises(AttributeError):
        unfit.CPOD(lim)


def test_knob_overruns_and_non_finite():
    case = make_case(**CASES['c1'])
    lim = {'limits': case['limits']}
    rom = fitted(case, cpod_max_rounds=1)
    with pytest.raises(RuntimeError, match='cpod_max_rounds'):
        rom.CPOD(lim)
    rom = fitted(case, cpod_max_rows=3)
    with pytest.raises(RuntimeError, match='cpod_max_rows'):
        rom.CPOD(lim)
    rom = fitted(case, cpod_rows_per_round=0)
    with pytest.raises(ValueError):
        rom.CPOD(lim)
    rom = fitted(case)
    rom.Ar = np.array(rom.Ar)
    rom.Ar[3, 2] = np.nan
    with pytest.raises(np.linalg.LinAlgError):
        rom.CPOD(lim)


def test_distance_qp_on_near_copies_far_from_the_centre():
    """the synthetic QP of the issue: 30 rows, 15 of them near-copies of the others, |a| ~ 100"""
    from openmeasure_amd._cpod import solve_distance_qp
    rng = np.random.default_rng(5)
    r = 12
    B = rng.standard_normal((15, r))
    A = np.vstack([B, B + 1e-7 * rng.standard_normal((15, r))])
    b = rng.uniform(0.001, 0.01, 30)                           # g = 0 is strictly feasible
    a = 100.0 * rng.standard_normal(r) / np.sqrt(r)
    g, lam = solve_distance_qp(a, A, b)
    assert np.all(lam >= 0)
    assert (A @ g - b).max() <= 1e-11
    assert np.abs(g - a + A.T @ lam).max() <= 1e-12 * np.abs(a).max()
    assert np.abs(lam * (A @ g - b)).max() <= 1e-12 * lam.max()
    g2, lam2 = solve_distance_qp(np.zeros(2), np.array([[1.0, 0.0], [-1.0, 0.0]]), np.array([-1.0, 0.5]))
    assert g2 is None and lam2 is None                         # x <= -1 and x >= -0.5


def test_cols_path_is_untouched():
    """train() takes the per-feature extremes of X_cnt from the helper CPOD shares"""
    case = make_case(seed=8, n_points=300, F=3, m=30, r=6)
    spr = fitted(case, cls=SPR)
    spr.train(spr.optimal_placement(), limits=case['limits'], method='COLS')
    cnt = np.asarray(spr.X_cnt)[:, 0].reshape(case['F'], -1)
    np.testing.assert_array_equal(spr._cols_cnt_minmax, np.stack([cnt.min(axis=1), cnt.max(axis=1)], axis=1))


def test_info_keys_and_overrun_messages_of_both_drivers():
    """cols_info_ and cpod_info_ keep their exact key sets (cols_info_ has no rows_seconds / cached_rows), and the
    *_max_rounds / *_max_rows RuntimeErrors of predict(method='COLS') and CPOD keep their full text: the figures in them
    (violation, violated rows) depend on the data and are matched by their format"""
    import re
    from tests.test_cols_host import measurements
    per_vector = {'status', 'rounds', 'rows', 'sides', 'multipliers', 'max_violation'}
    num, tol = r'\d\.\d{3}e[+-]\d{2}', re.escape('1.0e-09')
    case = make_case(**CASES['c1'])
    lim = {'limits': case['limits']}

    spr = fitted(case, cls=SPR)
    spr.train(spr.optimal_placement(), limits=case['limits'], method='COLS')
    y = measurements(case, spr.sensors_, 0)
    spr.predict(y)
    assert spr.cols_info_['status'] == ['optimal']             # a bound is active: the loop ran past its first sweep
    assert set(spr.cols_info_) == per_vector | {'vectors', 'sweeps', 'sweep_seconds', 'qp_seconds'}
    spr.cols_max_rounds = 1
    with pytest.raises(RuntimeError) as exc:
        spr.predict(y)
    assert re.fullmatch(rf'COLS: vector 0 still violates its limits by {num} \(tolerance {tol}, \d+ rows\) after '
                        r'cols_max_rounds = 1 sweeps', str(exc.value)), str(exc.value)
    spr.cols_max_rounds, spr.cols_max_rows = 60, 3
    with pytest.raises(RuntimeError) as exc:
        spr.predict(y)
    assert str(exc.value) == 'COLS: vector 0 needs more than cols_max_rows = 3 working rows'

    rom = fitted(case)
    rom.CPOD(lim)
    assert 'optimal' in rom.cpod_info_['status']
    assert set(rom.cpod_info_) == per_vector | {'vectors', 'sweeps', 'sweep_seconds', 'rows_seconds', 'qp_seconds',
                                                'cached_rows'}
    rom = fitted(case, cpod_max_rounds=1)
    with pytest.raises(RuntimeError) as exc:
        rom.CPOD(lim)
    assert re.fullmatch(rf'CPOD: snapshot 0 still violates its limits by {num} \(tolerance {tol}, \d+ rows\) after '
                        r'cpod_max_rounds = 1 sweeps', str(exc.value)), str(exc.value)
    rom = fitted(case, cpod_max_rows=3)
    with pytest.raises(RuntimeError) as exc:
        rom.CPOD(lim)
    assert str(exc.value) == 'CPOD: snapshot 0 needs more than cpod_max_rows = 3 working rows'


# ------------------------------------------------------------------------------------------------------ sharded, over gloo
def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from openmeasure_amd.sparse_sensing import ROM, RowShard
        from tests.test_cols_host import ColsNumpyEngine, make_case
        from tests.test_cpod_host import CASES
        case = make_case(**CASES['c2'])
        n = case['X'].shape[0]                                 # 900 rows, features of 300: cut INSIDE a feature
        cuts = [0, 400, n]
        row0, n_loc = cuts[rank], cuts[rank + 1] - cuts[rank]
        rom = ROM(np.ascontiguousarray(case['X'][row0:row0 + n_loc]), case['F'], None, shard=RowShard(row0, n),
                  engine=ColsNumpyEngine())
        rom.fit(select_modes='number', n_modes=case['r'])
        calls = []
        ag = rom._all_gather
        rom._all_gather = lambda t: (calls.append('gather'), ag(t))[1]
        Ar0 = np.array(rom.Ar)
        rom.CPOD({'limits': case['limits']})
        info = rom.cpod_info_
        lo0, hi0 = rom.scale_limits(case['limits'])            # this rank's rows
        with open(os.path.join(out_dir, f'rank{rank}.pkl'), 'wb') as fh:
            pickle.dump(dict(Ar=rom.Ar, Ar0=Ar0, Ur=np.asarray(rom.Ur, dtype=np.float64), lo0=np.asarray(lo0),
                             hi0=np.asarray(hi0), tol=rom.cpod_tol, sweeps=info['sweeps'], gathers=calls.count('gather'),
                             info={k: info[k] for k in ('status', 'rounds', 'rows', 'sides', 'multipliers',
                                                        'max_violation')}), fh)
    finally:
        dist.destroy_process_group()


def test_sharded_cpod_over_gloo(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    got = []
    for q in range(2):
        with open(tmp_path / f'rank{q}.pkl', 'rb') as fh:
            got.append(pickle.load(fh))
    case = make_case(**CASES['c2'])
    rom = fitted(case)
    rom.CPOD({'limits': case['limits']})
    # the sharded answer on the FULL problem, evaluated here from the ranks' own blocks of Ur and of the scaled limits: a
    # binding row the other rank missed would fail feasibility, a wrong multiplier stationarity -- at the bars of (i)
    U = np.vstack([g['Ur'] for g in got])
    lo0, hi0 = np.concatenate([g['lo0'] for g in got]), np.concatenate([g['hi0'] for g in got])
    assert U.shape == (case['X'].shape[0], case['r']) and lo0.shape == hi0.shape == (U.shape[0],)
    s_lo, s_hi = rom.scale_limits(case['limits'])
    np.testing.assert_allclose(lo0, s_lo, rtol=1e-12, atol=1e-12)          # the same limits as the single process scales
    np.testing.assert_allclose(hi0, s_hi, rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(got[1]['Ar0'], got[0]['Ar0'])
    for q in range(2):
        np.testing.assert_array_equal(got[q]['Ar'], got[0]['Ar'])           # every rank solves the identical QPs
        assert got[q]['info']['status'] == ['optimal'] * case['X'].shape[1]
        kkt_check(U, lo0, hi0, got[q]['tol'], got[q]['Ar'], got[q]['Ar0'], got[q]['info'], tag=f'CPOD sharded rank {q}')
        diff = np.abs(got[q]['Ar'] - rom.Ar).max()
        print('CPOD sharded - single', diff, 'bar', same_bar(rom, rom._cpod_Ar0))
        assert diff <= same_bar(rom, rom._cpod_Ar0)
        assert got[q]['gathers'] == got[q]['sweeps'] + 1                    # one per round + the extremes of X_cnt
