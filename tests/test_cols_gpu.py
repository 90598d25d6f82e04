"""train(method='COLS') on the HIP engine: the bound-sweep kernel (csrc/bounds.hip) against NumPy, and the whole
fit -> optimal_placement -> train(limits, 'COLS') -> predict -> reconstruct chain against the KKT conditions and SciPy's
SLSQP on the full constraint set.  Yardsticks, their derivation and the bars are those of tests/test_cols_host.py
(measured there on an exact host solve; the HIP path is allowed the same 10 x: STAT_BAR 7e-15, COMP_BAR 3e-15,
SLSQP_BAR 7e-8)."""
import numpy as np
import pytest

from tests.test_cols_host import (CASES, EPS, _feas_round, check_against_yardsticks, kkt, make_case, measurements,
                                  problem, scaled_limits, trained)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    from openmeasure_amd.engine import HipEngine
    return HipEngine('cuda:0')


def _sweep_case(eng, r, n_p, dtype, seed, ldu_pad=0, clamp_feature=False):
    """a block that starts inside feature 1 of 4 and ends inside feature 3; n no multiple of any tile"""
    import torch
    rng = np.random.default_rng(seed)
    n_points, F = 1237, 4
    row0, n = 1237 + 411, 2 * 1237 + 389
    U = rng.standard_normal((n, r)) / np.sqrt(r)
    if dtype == 'f32':
        U = U.astype(np.float32)
    Upad = np.zeros((n, r + ldu_pad), dtype=U.dtype)
    Upad[:, :r] = U
    Ud = eng.to_device(Upad, dtype=torch.float32 if dtype == 'f32' else torch.float64)[:, :r]
    mu = rng.standard_normal(n) * 0.3
    scale = rng.uniform(0.5, 2.0, F)
    G = rng.standard_normal((n_p, r))
    limits = np.stack([-rng.uniform(1.0, 2.5, F), rng.uniform(1.0, 2.5, F)])
    clamp = np.full((2, F), np.nan)
    if clamp_feature:
        clamp[1, 2], clamp[0, 1] = 1000.0, -1000.0
    return dict(U=U.astype(np.float64), Ud=Ud, mu=mu, scale=scale, G=G, limits=limits, clamp=clamp, row0=row0, n=n,
                n_points=n_points, F=F)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('r,n_p,ldu_pad,clamped', [(3, 1, 0, False), (6, 5, 2, False), (64, 17, 0, True), (130, 5, 6, False),
                                                   (64, 1, 8, False), (6, 17, 0, True), (130, 1, 0, True), (3, 5, 1, True)])
def test_bound_sweep_against_numpy(eng, dtype, r, n_p, ldu_pad, clamped):
    c = _sweep_case(eng, r, n_p, dtype, seed=100 + r + n_p, ldu_pad=ldu_pad, clamp_feature=clamped)
    assert c['Ud'].stride(0) == r + ldu_pad
    tol, k = 0.05, 24
    out = eng.to_host(eng.bound_sweep(c['Ud'], c['row0'], c['n_points'], c['F'], eng.to_device(c['mu']), eng.to_device(c['scale']),
                                      eng.to_device(c['limits']), eng.to_device(c['clamp']), eng.to_device(c['G']), tol, k))
    assert out.shape == (n_p, 3 + 3 * k)
    lo0, hi0, feat = scaled_limits(c['row0'], c['n'], c['n_points'], c['F'], c['mu'], c['scale'], c['limits'], c['clamp'])
    for p in range(n_p):
        g = c['G'][p]
        x = c['U'] @ g
        v2 = np.stack([lo0 - x, x - hi0], axis=1)
        v = v2.max(axis=1)
        rnd = _feas_round(c['U'], g)                              # two summation orders of the same dot product
        assert abs(out[p, 0] - v.max()) <= rnd
        row = int(out[p, 1]) - c['row0']
        assert 0 <= row < c['n'] and v[row] >= v.max() - rnd    # the row it names attains the maximum (to rounding)
        sure, maybe = np.count_nonzero(v > tol + rnd), np.count_nonzero(v > tol - rnd)
        assert sure <= int(out[p, 2]) <= maybe
        cand = out[p, 3:].reshape(k, 3)
        used = cand[cand[:, 0] >= 0]
        assert np.all(cand[len(used):, 0] == -1) and np.all(np.isneginf(cand[len(used):, 2]))
        if v.max() <= tol - rnd:
            assert len(used) == 0 and int(out[p, 2]) == 0         # nothing violated: no candidates
            continue
        if len(used) == 0:
            assert v.max() <= tol + rnd
            continue
        assert int(used[0, 0]) == int(out[p, 1]) and used[0, 2] == out[p, 0]      # the global worst is the first candidate
        assert np.all(np.diff(used[:, 2]) <= 0)                                  # worst first
        keys = set()
        for rw, side, val in used:
            i, sd = int(rw) - c['row0'], int(side)
            assert 0 <= i < c['n'] and sd in (0, 1) and (i, sd) not in keys
            keys.add((i, sd))
            assert abs(v2[i, sd] - val) <= rnd and val > tol                    # every candidate is really violated


def test_bound_sweep_is_deterministic_and_validates(eng):
    c = _sweep_case(eng, 12, 3, 'f64', seed=5)
    args = (c['Ud'], c['row0'], c['n_points'], c['F'], eng.to_device(c['mu']), eng.to_device(c['scale']),
            eng.to_device(c['limits']), eng.to_device(c['clamp']), eng.to_device(c['G']))
    a = eng.to_host(eng.bound_sweep(*args, 0.01, 8))
    b = eng.to_host(eng.bound_sweep(*args, 0.01, 8))
    assert np.array_equal(a, b)
    with pytest.raises(ValueError):
        eng.bound_sweep(*args, 0.01, 0)
    with pytest.raises(ValueError):
        eng.bound_sweep(*args, -1.0, 8)


@pytest.mark.parametrize('name', sorted(CASES))
def test_end_to_end_against_kkt_and_slsqp(eng, name):
    case = make_case(**CASES[name])
    spr, C = trained(case, eng)
    y = measurements(case, spr.sensors_, 0)
    Ar, As = spr.predict(y)
    assert spr.cols_info_['status'] == ['optimal'] and spr.cols_info_['rounds'][0] >= 2
    check_against_yardsticks(spr, [y], Ar)
    xr = spr.reconstruct(Ar)
    for f in range(case['F']):
        blk = xr[f * case['n_points']:(f + 1) * case['n_points']]
        delta = spr.cols_tol * spr._scl_f[f] + 8 * EPS * max(abs(case['limits'][0][f]), abs(case['limits'][1][f]), 1.0) \
            + _feas_round(np.asarray(spr.Ur), Ar[0]) * spr._scl_f[f]
        assert blk.min() >= case['limits'][0][f] - delta and blk.max() <= case['limits'][1][f] + delta
    spr.train(C)
    A0, S0 = spr.predict(y)
    assert not np.array_equal(A0, Ar) and np.array_equal(S0, As)


def test_end_to_end_batch_non_binding_and_infeasible(eng):
    case = make_case(seed=8, n_points=400, F=3, m=30, r=6)
    wide = [case['limits'][0] - 50.0, case['limits'][1] + 50.0]
    spr, C = trained(case, eng, limits=wide)
    ys = [measurements(case, spr.sensors_, t) for t in range(3)]
    Ar, As = spr.predict(ys)
    assert spr.cols_info_['status'] == ['ols'] * 3 and spr.cols_info_['sweeps'] == 1
    spr.train(C)
    A0, S0 = spr.predict(ys)
    assert np.array_equal(Ar, A0) and np.array_equal(As, S0)            # bit-equal OLS
    spr.train(C, limits=case['limits'], method='COLS')
    Ab, _ = spr.predict(ys)
    assert spr.cols_info_['sweeps'] == max(spr.cols_info_['rounds']) and 'optimal' in spr.cols_info_['status']
    check_against_yardsticks(spr, ys, Ab)
    bad = [case['limits'][0].copy(), case['limits'][1].copy()]
    bad[0][1], bad[1][1] = bad[1][1], bad[0][1]                         # lo > hi on feature 1
    spr.train(C, limits=bad, method='COLS')
    An, Sn = spr.predict(ys)
    assert spr.cols_info_['status'] == ['infeasible'] * 3 and np.all(np.isnan(An)) and np.array_equal(Sn, S0)
    spr.train(C, limits=None, method='COLS')
    with pytest.raises(TypeError, match="'NoneType' object is not iterable"):
        spr.predict(ys)


def test_two_million_rows_kkt_only(eng):
    """n = 2.4e6 rows (eng.synth), r = 16: limits that cut the unconstrained solution's range by 10 %; KKT only"""
    from openmeasure_amd.rom import DeviceMatrix
    from openmeasure_amd.sparse_sensing import SPR
    from openmeasure_amd.synth import make_R
    n_points, F, m, r = 800_000, 3, 32, 16
    Xd = eng.synth(n_points * F, m, 0, n_points, eng.to_device(make_R(m, r, seed=7)), 1e-3, 7)
    spr = SPR(DeviceMatrix(Xd), F, None, engine=eng)
    spr.fit(select_modes='number', n_modes=r)
    C = spr.optimal_placement()
    spr.train(C)
    piv = spr.sensors_
    col = eng.to_host(Xd[:, 3].contiguous()).astype(np.float64)
    rng = np.random.default_rng(3)
    y = np.zeros((len(piv), 3))
    y[:, 0] = col[piv] + 0.05 * np.abs(col[piv]).max() * rng.standard_normal(len(piv))
    y[:, 2] = piv // n_points
    a0, _ = spr.predict(y)
    x0 = spr.reconstruct(a0)[:, 0]
    lo = np.array([x0[f * n_points:(f + 1) * n_points].min() for f in range(F)])
    hi = np.array([x0[f * n_points:(f + 1) * n_points].max() for f in range(F)])
    limits = [lo + 0.05 * (hi - lo), hi - 0.05 * (hi - lo)]
    spr.train(C, limits=limits, method='COLS')
    Ar, _ = spr.predict(y)
    info = spr.cols_info_
    print('COLS 2.4e6 rows:', info['status'], info['rounds'], [len(x) for x in info['rows']], info['max_violation'],
          f"sweep {info['sweep_seconds']:.3f} s qp {info['qp_seconds']:.3f} s")
    assert info['status'] == ['optimal'] and info['rounds'][0] >= 2
    k = kkt(problem(spr, y), Ar[0], info, 0, spr.cols_tol)
    print('COLS 2.4e6 rows KKT:', k)
    from tests.test_cols_host import COMP_BAR, STAT_BAR
    assert k['stat'] <= STAT_BAR and k['comp'] <= COMP_BAR, k
