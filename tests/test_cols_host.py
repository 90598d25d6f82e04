"""train(method='COLS') -> predict(): the constraint-generation loop and the working-set QP (openmeasure_amd/_cols.py)
on the CPU.  The bound sweep -- the one piece that is a HIP kernel in the product -- is supplied by ColsNumpyEngine below,
a NumPy bound_sweep of the same contract on top of the test double (tests/numpy_engine.py stays as it is).

Yardsticks (neither is the code under test, neither is the reference: cvxpy cannot be installed here):
 (i)  the KKT conditions of the full problem, evaluated here in NumPy f64 from Ur, Theta, y0, the returned g and
      cols_info_: feasibility over all n rows, multipliers >= 0, stationarity H g - f + A^T lambda, complementarity.
      H is positive definite, so a point that satisfies them is THE solution;
 (ii) SciPy's SLSQP on the full 2 n constraints (n <= 2 000), written in this file.

Bars.  Feasibility: max_violation <= cols_tol as reported; recomputed here <= cols_tol + FEAS_ROUND, the rounding of an
r-term f64 dot product |u|.|g| re-summed in another order: 2 r eps |u|_2 |g|_2 (derived in _feas_round).
Stationarity / complementarity (relative to |f|_inf resp. to lambda_max) and |g - g_SLSQP|_inf / |g|_inf: measured
on this very loop (exact host solve + NumPy sweep) over the six seeded shapes below and the batch / clamp cases:
    stationarity   1.6e-16 ... 6.3e-16     complementarity 1e-19 ... 2.8e-16     |g - g_SLSQP| / |g|   1.6e-15 ... 6.7e-9
(the last column is SLSQP's own accuracy at ftol = 1e-15, started from the unconstrained solution; rounds 3 ... 7,
working rows 9 ... 59.)  The bars are 10 x the worst measured figure, for another summation order in the sweep (the
MFMA kernel):
    STAT_BAR = 7e-15       COMP_BAR = 3e-15       SLSQP_BAR = 7e-8
The GPU tests (tests/test_cols_gpu.py) hold the HIP path to the same bars."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

from openmeasure_amd.sparse_sensing import SPR
from tests.numpy_engine import NumpyEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
STAT_BAR, COMP_BAR, SLSQP_BAR = 7e-15, 3e-15, 7e-8


class ColsNumpyEngine(NumpyEngine):
    """NumpyEngine + a NumPy bound_sweep with the contract of HipEngine.bound_sweep: candidates are the worst row per
    side of every segment of `seg` consecutive local rows (cut at feature boundaries)."""
    seg = 37

    def bound_sweep(self, Ur, row0, n_points, n_features, rowmean, scale, limits, clamp, G, tol, k):
        return torch.from_numpy(numpy_bound_sweep(self._w(Ur), row0, n_points, n_features, rowmean.numpy(), scale.numpy(),
                                                  limits.numpy(), clamp.numpy(), G.numpy(), tol, k, self.seg))


def scaled_limits(row0, n, n_points, F, mu, scale, limits, clamp):
    feat = np.minimum((row0 + np.arange(n)) // n_points, F - 1)
    out = []
    for j in range(2):
        l0 = (limits[j][feat] - mu) / scale[feat]
        cl = clamp[j][feat]
        out.append(np.where(np.isnan(cl), l0, cl))
    return out[0], out[1], feat


def numpy_bound_sweep(U, row0, n_points, F, mu, scale, limits, clamp, G, tol, k, seg):
    n = U.shape[0]
    lo0, hi0, feat = scaled_limits(row0, n, n_points, F, mu, scale, limits, clamp)
    out = np.empty((G.shape[0], 3 + 3 * k))
    cuts = sorted(set(range(0, n, seg)) | {int(c) for c in np.flatnonzero(np.diff(feat)) + 1} | {n})
    for p, g in enumerate(G):
        x = U @ g
        v2 = np.stack([lo0 - x, x - hi0], axis=1)                 # side 0 = lower, 1 = upper
        v = v2.max(axis=1)
        i = int(np.argmax(v))                                     # first (lowest) row of the maximum
        cands = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            for side in (0, 1):
                j = a + int(np.argmax(v2[a:b, side]))
                if v2[j, side] > tol:
                    cands.append((row0 + j, side, v2[j, side]))
        cands.sort(key=lambda t: (-t[2], t[0], t[1]))
        rec = np.tile([-1.0, 0.0, -np.inf], k)
        for q, c in enumerate(cands[:k]):
            rec[3 * q:3 * q + 3] = c
        out[p, :3] = (v[i], row0 + i, np.count_nonzero(v > tol))
        out[p, 3:] = rec
    return out


# ---------------------------------------------------------------------------------------------------------------- data
def make_case(seed, n_points, F, m, r, noise=0.02, weighted=False, offset=0.0):
    """Gaussian bumps clipped at 0 (F features, feature-major), limits = per-feature min / max of the data (they bind:
    a truncated basis undershoots the clipped zero level), a noisy snapshot-like field to measure."""
    rng = np.random.default_rng(seed)
    xs = np.linspace(0.0, 1.0, n_points)
    X = np.empty((n_points * F, m))
    for j in range(m):
        for f in range(F):
            c, w, a = rng.uniform(0.15, 0.85), rng.uniform(0.03, 0.12), rng.uniform(0.5, 2.0) * (f + 1)
            X[f * n_points:(f + 1) * n_points, j] = np.clip(a * np.exp(-0.5 * ((xs - c) / w) ** 2) - 0.1 * a, 0.0, None) + offset
    lo = np.array([X[f * n_points:(f + 1) * n_points].min() for f in range(F)])
    hi = np.array([X[f * n_points:(f + 1) * n_points].max() for f in range(F)])
    truth = []
    for t in range(3):
        col = np.empty(n_points * F)
        for f in range(F):
            c, w, a = rng.uniform(0.15, 0.85), rng.uniform(0.03, 0.12), rng.uniform(0.5, 2.0) * (f + 1)
            col[f * n_points:(f + 1) * n_points] = np.clip(a * np.exp(-0.5 * ((xs - c) / w) ** 2) - 0.1 * a, 0.0, None) + offset
        truth.append(col)
    return dict(X=X, F=F, n_points=n_points, r=r, limits=[lo, hi], truth=truth, noise=noise, weighted=weighted, seed=seed)


def measurements(case, piv, t):
    rng = np.random.default_rng(1000 * case['seed'] + t)
    x = case['truth'][t]
    sig = case['noise'] * (1 + np.arange(len(piv)) % 3)
    y = np.zeros((len(piv), 3))
    y[:, 0] = x[piv] + sig * rng.standard_normal(len(piv))
    y[:, 1] = sig if case['weighted'] else 0.0
    y[:, 2] = piv // case['n_points']
    return y


def trained(case, engine, limits=None, n_sensors=None, **knobs):
    spr = SPR(case['X'], case['F'], None, engine=engine)
    spr.fit(select_modes='number', n_modes=case['r'])
    C = spr.optimal_placement()
    for k, v in knobs.items():
        setattr(spr, k, v)
    spr.train(C, limits=case['limits'] if limits is None else limits, method='COLS')
    return spr, C


# ------------------------------------------------------------------------------------------------------------ yardsticks
def problem(spr, y, y0=None):
    """H, f, scaled limits and the basis of the full problem, from the object's downloaded state, in NumPy f64."""
    Theta, Ur = np.asarray(spr.Theta, dtype=np.float64), np.asarray(spr.Ur, dtype=np.float64)
    y0 = spr.scale_vector(y) if y0 is None else y0
    w = 1.0 / y0[:, 1] if np.any(y[:, 1]) else np.ones(len(y0))
    WT = Theta * w[:, None]
    lo0, hi0 = spr.scale_limits(spr.limits)
    return dict(H=WT.T @ WT, f=WT.T @ (w * y0[:, 0]), U=Ur, lo0=lo0, hi0=hi0)


def _feas_round(U, g):
    """|fl(u.g) - fl'(u.g)| for two summation orders of an r-term f64 dot product: each is within r eps |u|.|g| of the
    exact value (Higham, Accuracy and Stability, (3.5), gamma_r ~ r eps), |u|.|g| <= |u|_2 |g|_2; both orders -> 2 x."""
    return 2 * U.shape[1] * EPS * np.sqrt((U * U).sum(axis=1)).max() * np.linalg.norm(g)


def kkt(pb, g, info, p, tol):
    """-> dict of the KKT residuals of vector p; asserts feasibility and the sign of the multipliers."""
    x = pb['U'] @ g
    viol = max((x - pb['hi0']).max(), (pb['lo0'] - x).max())
    assert info['max_violation'][p] <= tol
    assert viol <= tol + _feas_round(pb['U'], g), (viol, tol)
    rows, sides, lam = info['rows'][p], info['sides'][p], info['multipliers'][p]
    assert len(rows) == len(sides) == len(lam) and np.all(lam >= 0)
    sign = np.where(sides == 1, 1.0, -1.0)
    A = sign[:, None] * pb['U'][rows]
    b = np.where(sides == 1, pb['hi0'][rows], -pb['lo0'][rows])
    stat = np.abs(pb['H'] @ g - pb['f'] + A.T @ lam).max() / max(np.abs(pb['f']).max(), 1e-300)
    comp = np.abs(lam * (A @ g - b)).max() / max(lam.max(), 1e-300) if len(lam) else 0.0
    return dict(viol=viol, stat=stat, comp=comp, active=int(np.count_nonzero(lam > 0)))


def slsqp(pb, g0):
    from scipy.optimize import minimize
    H, f, U = pb['H'], pb['f'], pb['U']
    s = 1.0 / max(np.abs(f).max(), 1e-300)
    cons = [dict(type='ineq', fun=lambda g: pb['hi0'] - U @ g, jac=lambda g: -U),
            dict(type='ineq', fun=lambda g: U @ g - pb['lo0'], jac=lambda g: U)]
    res = minimize(lambda g: s * (0.5 * g @ H @ g - f @ g), g0, jac=lambda g: s * (H @ g - f), constraints=cons,
                   method='SLSQP', options=dict(ftol=1e-15, maxiter=500))
    assert res.success, res.message
    return res.x


def check_against_yardsticks(spr, ys, Ar, with_slsqp=True, min_rounds=2, report=None):
    info = spr.cols_info_
    for p, y in enumerate(ys):
        pb = problem(spr, y)
        k = kkt(pb, Ar[p], info, p, spr.cols_tol)
        line = dict(p=p, status=info['status'][p], rounds=info['rounds'][p], rows=len(info['rows'][p]), **k)
        assert info['status'][p] in ('optimal', 'ols')
        if info['status'][p] == 'optimal':
            assert info['rounds'][p] >= min_rounds and len(info['rows'][p]) > 0
        if with_slsqp and info['status'][p] == 'optimal':    # an 'ols' vector IS the OLS result (compared bit for bit elsewhere)
            gs = slsqp(pb, np.linalg.solve(pb['H'], pb['f']))      # started at the unconstrained solution, not at ours
            line['slsqp'] = np.abs(Ar[p] - gs).max() / np.abs(Ar[p]).max()
        print('COLS', line)
        if report is not None:
            report.append(line)
        assert k['stat'] <= STAT_BAR and k['comp'] <= COMP_BAR, line
        if 'slsqp' in line:
            assert line['slsqp'] <= SLSQP_BAR, line


# ----------------------------------------------------------------------------------------------------------------- tests
CASES = {
    'f3_r6': dict(seed=1, n_points=400, F=3, m=30, r=6),
    'f4_r12': dict(seed=2, n_points=500, F=4, m=40, r=12),
    'f1_r8': dict(seed=3, n_points=1500, F=1, m=30, r=8),
    'f3_r10_weighted': dict(seed=4, n_points=600, F=3, m=36, r=10, weighted=True),
    'f3_r16': dict(seed=5, n_points=650, F=3, m=48, r=16),
    'f4_r20_weighted': dict(seed=6, n_points=450, F=4, m=50, r=20, weighted=True),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_loop_against_kkt_and_slsqp(name):
    case = make_case(**CASES[name])
    spr, C = trained(case, ColsNumpyEngine())
    y = measurements(case, spr.sensors_, 0)
    ols = SPR(case['X'], case['F'], None, engine=NumpyEngine())
    ols.fit(select_modes='number', n_modes=case['r'])
    ols.train(ols.optimal_placement())
    g_ols, _ = ols.predict(y)
    Ar, As = spr.predict(y)
    assert Ar.shape == As.shape == (1, case['r'])
    assert spr.cols_info_['status'] == ['optimal'] and spr.cols_info_['rounds'][0] >= 2
    assert spr.cols_info_['sweeps'] == spr.cols_info_['rounds'][0]
    assert not np.array_equal(Ar, g_ols)                       # the limits bind: the OLS shortcut alone cannot pass
    np.testing.assert_array_equal(As, ols.predict(y)[1])       # Ar_sigma as in OLS
    check_against_yardsticks(spr, [y], Ar)
    xr = spr.reconstruct(Ar)                                   # the reconstructed field respects the limits
    for f in range(case['F']):
        blk = xr[f * case['n_points']:(f + 1) * case['n_points']]
        delta = spr.cols_tol * spr._scl_f[f] + 8 * EPS * max(abs(case['limits'][0][f]), abs(case['limits'][1][f]), 1.0) \
            + _feas_round(np.asarray(spr.Ur), Ar[0]) * spr._scl_f[f]
        assert blk.min() >= case['limits'][0][f] - delta and blk.max() <= case['limits'][1][f] + delta


def test_batch_of_three_one_needs_no_constraint():
    case = make_case(seed=7, n_points=500, F=3, m=30, r=8)
    spr, C = trained(case, ColsNumpyEngine())
    ys = [measurements(case, spr.sensors_, t) for t in range(2)]
    y_in = np.zeros((len(spr.sensors_), 3))                    # the sensors of a field that IS in the span and inside the limits:
    g_in = np.zeros(case['r'])                                 # the centre of the data (g = 0), where no row is at a limit
    y_in[:, 0], y_in[:, 2] = spr.reconstruct(g_in[None])[spr.sensors_, 0], spr.sensors_ // case['n_points']
    batch = [ys[0], y_in, ys[1]]
    Ar, As = spr.predict(batch)
    assert spr.cols_info_['status'] == ['optimal', 'ols', 'optimal'], spr.cols_info_['max_violation']
    assert spr.cols_info_['rounds'][1] == 1 and len(spr.cols_info_['rows'][1]) == 0
    assert spr.cols_info_['sweeps'] == max(spr.cols_info_['rounds'])      # all unfinished vectors share each sweep
    check_against_yardsticks(spr, batch, Ar)
    for p in (0, 2):                                                      # same answer alone as in the batch
        a1, _ = spr.predict(batch[p])
        np.testing.assert_array_equal(a1[0], Ar[p])
    spr.train(C)
    np.testing.assert_array_equal(spr.predict(y_in)[0][0], Ar[1])         # the OLS result itself


def test_non_binding_limits_return_the_ols_result_bit_for_bit():
    case = make_case(seed=8, n_points=400, F=3, m=30, r=6)
    wide = [case['limits'][0] - 50.0, case['limits'][1] + 50.0]
    spr, C = trained(case, ColsNumpyEngine(), limits=wide)
    ys = [measurements(case, spr.sensors_, t) for t in range(3)]
    Ar, As = spr.predict(ys)
    assert spr.cols_info_['status'] == ['ols'] * 3 and spr.cols_info_['rounds'] == [1] * 3 and spr.cols_info_['sweeps'] == 1
    spr.train(C)
    A0, S0 = spr.predict(ys)
    assert np.array_equal(Ar, A0) and np.array_equal(As, S0)


def test_clamped_feature():
    """a limit far outside the data: (limit - X_cnt) / X_scl > 1000 -> the reference substitutes 1000 for the whole
    feature block (:201-204); the other features' limits bind"""
    case = make_case(seed=9, n_points=500, F=3, m=30, r=8)
    lim = [case['limits'][0].copy(), case['limits'][1].copy()]
    spr0, _ = trained(case, ColsNumpyEngine())
    lim[1][1] = case['limits'][1][1] + 5000.0 * spr0._scl_f[1]
    lim[0][2] = case['limits'][0][2] - 5000.0 * spr0._scl_f[2]
    spr, C = trained(case, ColsNumpyEngine(), limits=lim)
    lo0, hi0 = spr.scale_limits(lim)
    n_pt = case['n_points']
    assert np.all(hi0[n_pt:2 * n_pt] == 1000) and np.all(lo0[2 * n_pt:] == -1000)
    y = measurements(case, spr.sensors_, 1)
    Ar, _ = spr.predict(y)
    assert spr.cols_info_['status'] == ['optimal'] and spr.cols_info_['rounds'][0] >= 2
    check_against_yardsticks(spr, [y], Ar)


def test_infeasible_limits_give_a_nan_row_and_leave_the_others_alone():
    case = make_case(seed=10, n_points=400, F=3, m=30, r=6)
    spr, C = trained(case, ColsNumpyEngine())
    ys = [measurements(case, spr.sensors_, t) for t in range(2)]
    good, _ = spr.predict(ys)
    bad = [case['limits'][0].copy(), case['limits'][1].copy()]
    bad[0][1], bad[1][1] = bad[1][1], bad[0][1]                # lo > hi on feature 1
    spr.train(C, limits=bad, method='COLS')
    Ar, As = spr.predict(ys)
    assert spr.cols_info_['status'] == ['infeasible', 'infeasible'] and np.all(np.isnan(Ar))
    spr.train(C)
    np.testing.assert_array_equal(As, spr.predict(ys)[1])
    # a batch where only one vector is infeasible cannot be built from limits (they are shared): instead check that the
    # feasible problem's answers do not depend on what else was solved in the object before
    spr.train(C, limits=case['limits'], method='COLS')
    again, _ = spr.predict(ys)
    np.testing.assert_array_equal(again, good)


def test_argument_errors_and_refusals():
    case = make_case(seed=11, n_points=300, F=3, m=30, r=6)
    spr, C = trained(case, ColsNumpyEngine())
    y = measurements(case, spr.sensors_, 0)
    spr.train(C, limits=None, method='COLS')                   # the reference stores None and fails in predict (:883)
    with pytest.raises(TypeError, match="'NoneType' object is not iterable"):
        spr.predict(y)
    with pytest.raises(ValueError, match='number of rows of Theta'):
        spr.predict(y[:-1])
    spr.train(C[:4], limits=case['limits'], method='COLS')     # s = 4 < r = 6
    with pytest.raises(NotImplementedError, match='not unique'):
        spr.predict(y[:4])
    spr.train(C, limits=case['limits'], method='COLS')
    spr.cols_max_rounds = 1
    with pytest.raises(RuntimeError, match='cols_max_rounds'):
        spr.predict(y)
    spr.cols_max_rounds, spr.cols_max_rows = 60, 3
    with pytest.raises(RuntimeError, match='cols_max_rows'):
        spr.predict(y)
    plain = SPR(case['X'], case['F'], None, engine=NumpyEngine())          # no bound_sweep: no CPU fallback
    plain.fit(select_modes='number', n_modes=6)
    with pytest.raises(NotImplementedError):
        plain.train(plain.optimal_placement(), limits=case['limits'], method='COLS')


def test_working_qp_against_slsqp_on_random_problems():
    from scipy.optimize import minimize
    from openmeasure_amd._cols import solve_working_qp
    rng = np.random.default_rng(12)
    for trial in range(20):
        r, mc = int(rng.integers(2, 12)), int(rng.integers(1, 40))
        B = rng.standard_normal((r + 5, r))
        H, f = B.T @ B, rng.standard_normal(r)
        A, b = rng.standard_normal((mc, r)), rng.uniform(0.05, 1.0, mc)        # g = 0 is strictly feasible
        L = np.linalg.cholesky(H)
        g, lam = solve_working_qp(L, np.linalg.solve(H, f), A, b)
        assert np.all(lam >= 0) and (A @ g - b).max() <= 1e-12
        assert np.abs(H @ g - f + A.T @ lam).max() <= 1e-12 * max(1.0, np.abs(f).max()) * np.linalg.cond(H)
        res = minimize(lambda x: 0.5 * x @ H @ x - f @ x, np.zeros(r), jac=lambda x: H @ x - f, method='SLSQP',
                       constraints=[dict(type='ineq', fun=lambda x: b - A @ x, jac=lambda x: -A)],
                       options=dict(ftol=1e-15, maxiter=500))
        assert np.abs(res.x - g).max() <= 1e-6 * max(1.0, np.abs(g).max())
    g, lam = solve_working_qp(np.eye(2), np.zeros(2), np.array([[1.0, 0.0], [-1.0, 0.0]]), np.array([-1.0, 0.5]))
    assert g is None and lam is None                                          # x <= -1 and x >= -0.5


# ------------------------------------------------------------------------------------------------------ sharded, over gloo
def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from openmeasure_amd.sparse_sensing import SPR, RowShard
        from tests.test_cols_host import CASES, ColsNumpyEngine, make_case, measurements
        case = make_case(**CASES['f3_r10_weighted'])
        n = case['X'].shape[0]                                 # 1800 rows, features of 600: equal blocks of 900 / 600 ...
        cuts = [0, 700, n] if world == 2 else [0, 500, 1300, n]   # ... so cut by hand INSIDE features
        row0, n_loc = cuts[rank], cuts[rank + 1] - cuts[rank]
        spr = SPR(np.ascontiguousarray(case['X'][row0:row0 + n_loc]), case['F'], None, shard=RowShard(row0, n),
                  engine=ColsNumpyEngine())
        spr.fit(select_modes='number', n_modes=case['r'])
        C = spr.optimal_placement()
        spr.train(C, limits=case['limits'], method='COLS')
        ys = [measurements(case, spr.sensors_, t) for t in range(2)]
        calls = []
        ag, ar = spr._all_gather, spr._all_reduce
        spr._all_gather = lambda t: (calls.append('gather'), ag(t))[1]
        spr._all_reduce = lambda t: (calls.append('reduce'), ar(t))[1]
        Ar, As = spr.predict(ys)
        info = spr.cols_info_
        grown = sum(max(0, r - 1) for r in [max(info['rounds'])])          # rounds in which rows were added
        np.savez(os.path.join(out_dir, f'rank{rank}.npz'), Ar=Ar, As=As, sweeps=info['sweeps'],
                 gathers=calls.count('gather'), reduces=calls.count('reduce'), grown=grown,
                 rounds=np.asarray(info['rounds']))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('world', [2, 3])
def test_sharded_cols_over_gloo(tmp_path, world):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    got = [np.load(tmp_path / f'rank{q}.npz') for q in range(world)]
    case = make_case(**CASES['f3_r10_weighted'])
    spr, C = trained(case, ColsNumpyEngine())
    ys = [measurements(case, spr.sensors_, t) for t in range(2)]
    Ar, As = spr.predict(ys)
    assert min(spr.cols_info_['rounds']) >= 2
    for q in range(world):
        np.testing.assert_array_equal(got[q]['Ar'], got[0]['Ar'])           # every rank solves the identical QP
        assert np.abs(got[q]['Ar'] - Ar).max() <= SLSQP_BAR * np.abs(Ar).max()
        assert min(got[q]['rounds']) >= 2
        # per round: ONE all-gather (the sweep records); per round that adds rows: TWO all-reduces (rows of Ur, X_cnt)
        assert got[q]['gathers'] == got[q]['sweeps']
        assert got[q]['reduces'] <= 2 * got[q]['grown'] and got[q]['reduces'] >= 2
    shard = SPR(case['X'], case['F'], None, engine=ColsNumpyEngine())      # the sharded answer satisfies the KKT conditions
    shard.fit(select_modes='number', n_modes=case['r'])
    shard.train(shard.optimal_placement(), limits=case['limits'], method='COLS')
    for p, y in enumerate(ys):
        pb = problem(shard, y)
        x = pb['U'] @ got[0]['Ar'][p]
        assert max((x - pb['hi0']).max(), (pb['lo0'] - x).max()) <= shard.cols_tol + 10 * _feas_round(pb['U'], Ar[p])
