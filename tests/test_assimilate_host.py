"""SPR.assimilate on the CPU: the public method over a NumPy double of the engine call (HipEngine.assimilate,
csrc/assimilate.hip, held to the same oracle in tests/test_assimilate_gpu.py).

The double and the kernel use the INFORMATION form  H' = I + B^T B,  z = H'^-1 B^T W res,  a = a0 + C z,  F = C L'^-T.
The oracle uses the other formulation, the KALMAN form, in np.longdouble with a hand-written Cholesky:
    M = Theta S0 Theta^T + R,   a = a0 + S0 Theta^T M^-1 res,   cov = S0 - S0 Theta^T M^-1 Theta S0,
    chi2 = res^T M^-1 res,   logdet = log det M,   z = C^T Theta^T M^-1 res  (push-through identity).

Bars (the same on the device): with eps = 2^-52 and kappa = cond_2(H') computed from the oracle's matrices,
    |z - z_ref|_2 <= 16 (s + q) eps kappa |z_ref|_2,  |F F^T - cov_ref|_F <= the same multiple of |cov_ref|_F,
    |chi2 - ref| <= the same multiple of |W res|^2,  |logdet - ref| <= the same multiple of (q + sum |log sig0^2|).
The posterior mean is compared through z = C^+ (a - a0) where C has full column rank, which adds the rounding of a0 + C z:
eps |a| |C^+| -- the inputs are drawn with |a0| ~ |C z| so that this stays inside the bar's factor 16 (s + q) >= 32.
"""
import os
import sys

import numpy as np
import pytest
import torch

from openmeasure_amd.sparse_sensing import SPR
from tests.test_field_std_host import FieldStdNumpyEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
EPS = 2.0 ** -52


# ------------------------------------------------------------------------------------------------ the oracle (Kalman form)
def chol_lower(K):
    m = len(K)
    L = np.zeros_like(K)
    for j in range(m):
        L[j, j] = np.sqrt(K[j, j] - L[j, :j] @ L[j, :j])
        L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def chol_solve(L, Bm):
    """(L L^T)^-1 Bm by two substitutions, in L's dtype; Bm (m,) or (m, k)"""
    X = np.array(Bm, dtype=L.dtype)
    m = len(L)
    for j in range(m):
        X[j] = (X[j] - L[j, :j] @ X[:j]) / L[j, j]
    for j in range(m - 1, -1, -1):
        X[j] = (X[j] - L[j + 1:, j] @ X[j + 1:]) / L[j, j]
    return X


def kalman_oracle(Theta, y0, sig0, a0, C):
    """One vector, longdouble.  -> dict(a, cov, z, chi2, logdet, kappa, wres2, logabs)"""
    Th, y0, sig0, a0, C = (np.asarray(x, dtype=LD) for x in (Theta, y0, sig0, a0, C))
    S0 = C @ C.T
    M = Th @ S0 @ Th.T + np.diag(sig0 * sig0)
    Lm = chol_lower(M)
    res = y0 - Th @ a0
    Mr = chol_solve(Lm, res)
    G = chol_solve(Lm, Th @ S0)
    B = (Th / sig0[:, None]) @ C
    Hp = np.eye(C.shape[1]) + (B.T @ B).astype(np.float64)
    return dict(a=a0 + S0 @ (Th.T @ Mr), cov=S0 - S0 @ Th.T @ G, z=C.T @ (Th.T @ Mr), chi2=res @ Mr,
                logdet=2 * np.sum(np.log(np.diag(Lm))), kappa=np.linalg.cond(Hp), wres2=float(np.sum((res / sig0) ** 2)),
                logabs=float(np.sum(np.abs(np.log(sig0 * sig0)))))


def bar_factor(s, q, kappa):
    return 16 * (s + q) * EPS * kappa


def check_vector(ref, s, q, z=None, F=None, chi2=None, logdet=None):
    """the four bars of the module docstring -> the worst error / bar ratio"""
    m = bar_factor(s, q, ref['kappa'])
    worst = 0.0
    if z is not None:
        worst = max(worst, float(np.linalg.norm(z - ref['z']) / max(m * np.linalg.norm(ref['z']), 1e-300)))
    if F is not None:
        cov = np.asarray(F, dtype=LD) @ np.asarray(F, dtype=LD).T
        nrm = float(np.linalg.norm(ref['cov']))
        err = float(np.linalg.norm(cov - ref['cov']))
        worst = max(worst, err / (m * nrm) if nrm > 0 else (0.0 if err == 0 else np.inf))
    if chi2 is not None:
        worst = max(worst, float(abs(chi2 - ref['chi2'])) / (m * ref['wres2']))
    if logdet is not None:
        worst = max(worst, float(abs(logdet - ref['logdet'])) / (m * (q + ref['logabs'])))
    return worst


# ------------------------------------------------------------------------------------------------ the engine double
def numpy_assimilate(Th, c, sc, Y, a0, S=None, L=None):
    """the contract of HipEngine.assimilate in float64 NumPy, information form"""
    n_p, s, r = Y.shape[0], Th.shape[0], Th.shape[1]
    q = r if L is None else L.shape[2]
    Ar, As, F = np.zeros((n_p, r)), np.zeros((n_p, r)), np.zeros((n_p, r, q))
    info, Z = np.zeros((n_p, 4)), np.zeros((n_p, q))
    for p in range(n_p):
        scl = sc[Y[p, :, 2].astype(int)]
        y0, sig0 = (Y[p, :, 0] - c) / scl, Y[p, :, 1] / scl
        w = 1.0 / sig0
        C = np.diag(S[p]) if L is None else L[p]
        B = (w[:, None] * Th) @ C
        b = w * (y0 - Th @ a0[p])
        Lc = np.linalg.cholesky(np.eye(q) + B.T @ B)
        X = np.linalg.solve(Lc, np.eye(q))
        u = X @ (B.T @ b)
        Z[p] = X.T @ u
        m = C @ Z[p]
        Ar[p] = np.where(m == 0, a0[p], a0[p] + m)
        F[p] = C @ X.T
        As[p] = np.sqrt(np.sum(F[p] * F[p], axis=1))
        d = np.diag(Lc)
        info[p] = (0 if np.all(np.isfinite(w)) else 2, (d.max() / d.min()) ** 2, b @ b - u @ u,
                   np.sum(np.log(sig0 * sig0)) + 2 * np.sum(np.log(d)))
    return Ar, As, F, info, Z


class AssimNumpyEngine(FieldStdNumpyEngine):
    """NumpyEngine + field_std + a NumPy assimilate with the contract of HipEngine's; counts its calls"""
    assim_calls = 0

    def assimilate(self, Theta, cnt, scale, y, a0, S=None, L=None):
        assert (S is None) != (L is None)
        s, r = Theta.shape
        n_p = y.shape[0]
        assert n_p >= 1 and r <= 128 and tuple(y.shape) == (n_p, s, 3) and tuple(a0.shape) == (n_p, r)
        assert all(x is None or x.dtype == torch.float64 for x in (y, a0, S, L))
        if S is not None:
            assert tuple(S.shape) == (n_p, r)
        else:
            assert L.dim() == 3 and tuple(L.shape[:2]) == (n_p, r) and 1 <= L.shape[2] <= r
        self.assim_calls += 1
        out = numpy_assimilate(Theta.numpy(), cnt.numpy(), scale.numpy(), y.numpy(), a0.numpy(),
                               None if S is None else S.numpy(), None if L is None else L.numpy())
        return tuple(torch.from_numpy(np.ascontiguousarray(x)) for x in out)


# ------------------------------------------------------------------------------------------------ cases
def make_field(seed=0, n_points=40, F=3, m=12):
    """F features of very different size (so that their scl differ) on n_points cells, m snapshots"""
    rng = np.random.default_rng(seed)
    xs = np.linspace(0, 1, n_points)
    modes = np.stack([np.sin((k + 1) * np.pi * xs + 0.3 * k) for k in range(8)], axis=1)
    X = np.concatenate([(10.0 ** f) * (modes @ rng.standard_normal((8, m))) + 5.0 * f for f in range(F)])
    return X


def trained_spr(s, r=6, seed=0, engine=None, rows=None, **field):
    X = make_field(seed, **field)
    spr = SPR(X, field.get('F', 3), None, engine=engine or AssimNumpyEngine())
    spr.fit(select_modes='number', n_modes=r)
    rng = np.random.default_rng(seed + 1)
    rows = np.sort(rng.choice(X.shape[0], size=s, replace=False)) if rows is None else np.asarray(rows)
    C = np.zeros((s, X.shape[0]))
    C[np.arange(s), rows] = 1.0
    spr.train(C)
    return spr, rows


def draw_problem(spr, rows, n_p, seed=0, q=None, sensor_noise=0.05, zero_sigma=None):
    """prior (a0, C) and readings y consistent with it: a_true = a0 + C xi, y = field(a_true)[rows] + noise, in physical
    units.  q None: diagonal prior (C = diag(sigma))."""
    rng = np.random.default_rng(seed)
    r, s = spr.r, len(rows)
    Theta = np.asarray(spr.Theta)
    scl = spr._scl_f[rows // spr.n_points]
    cnt = spr._engine().to_host(spr._d['cnt'])
    a0 = rng.standard_normal((n_p, r))
    if q is None:
        sigma = rng.uniform(0.3, 2.0, (n_p, r))
        if zero_sigma is not None:
            sigma[zero_sigma] = 0.0
        Cs = np.stack([np.diag(sg) for sg in sigma])
    else:
        sigma = None
        Cs = np.stack([np.linalg.qr(rng.standard_normal((r, q)))[0] * rng.uniform(0.5, 2.0, q) for _ in range(n_p)])
    ys = []
    for p in range(n_p):
        a_true = a0[p] + Cs[p] @ rng.standard_normal(Cs[p].shape[1])
        sig0 = sensor_noise * rng.uniform(0.5, 2.0, s)
        y0 = Theta @ a_true + sig0 * rng.standard_normal(s)
        ys.append(np.stack([y0 * scl + cnt, sig0 * scl, (rows // spr.n_points).astype(float)], axis=1))
    return ys, a0, sigma, Cs


def scaled(spr, rows, y):
    scl = spr._scl_f[rows // spr.n_points]
    cnt = spr._engine().to_host(spr._d['cnt'])
    return (y[:, 0] - cnt) / scl, y[:, 1] / scl


def check_against_oracle(spr, rows, ys, a0, Cs, out, tag):
    Ar, Ar_std, F = out
    info = spr.assimilate_info_
    Theta = np.asarray(spr.Theta)
    s, q = Theta.shape[0], Cs[0].shape[1]
    worst = 0.0
    for p, y in enumerate(ys):
        y0, sig0 = scaled(spr, rows, y)
        ref = kalman_oracle(Theta, y0, sig0, a0[p], Cs[p])
        z = np.linalg.pinv(Cs[p]) @ (Ar[p] - a0[p])
        w = check_vector(ref, s, q, z=z, F=F[p], chi2=info['chi2'][p], logdet=info['logdet'][p])
        worst = max(worst, w)
        np.testing.assert_allclose(Ar_std[p], np.sqrt(np.diag(F[p] @ F[p].T)), rtol=8 * q * EPS, atol=0)
    print(f'{tag}: worst error / bar {worst:.3e}')
    assert worst <= 1.0
    assert np.all(info['status'] == 0) and np.all(info['dof'] == s) and np.all(info['cond'] >= 1.0)


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize('s,q', [(9, None), (9, 6), (9, 3), (9, 1), (4, None), (4, 5)])
def test_class_over_the_double_against_the_kalman_oracle(s, q):
    spr, rows = trained_spr(s)
    ys, a0, sigma, Cs = draw_problem(spr, rows, 3, seed=s, q=q)
    if q is None:
        out = spr.assimilate(ys, a0, sigma)
        assert spr.assimilate_info_['prior'] == 'sigma'
    else:
        out = spr.assimilate(ys, a0, prior_factor=Cs)
        assert spr.assimilate_info_['prior'] == 'factor'
    assert out[0].shape == (3, 6) and out[1].shape == (3, 6) and out[2].shape == (3, 6, 6 if q is None else q)
    assert all(isinstance(x, np.ndarray) and x.dtype == np.float64 for x in out)
    check_against_oracle(spr, rows, ys, a0, Cs, out, f's={s} q={q}')


def test_fewer_sensors_than_modes_is_well_posed():
    spr, rows = trained_spr(2)
    ys, a0, sigma, Cs = draw_problem(spr, rows, 2, seed=5)
    out = spr.assimilate(ys, a0, sigma)
    check_against_oracle(spr, rows, ys, a0, Cs, out, 's=2 < r=6')
    assert np.all(out[1] <= sigma * (1 + 8 * EPS))          # sensors never increase a marginal deviation


def test_features_of_different_scale_and_a_negative_feature_id():
    spr, rows = trained_spr(12)
    assert len(set(np.round(np.log10(spr._scl_f)))) == 3 and len(set(rows // spr.n_points)) == 3
    ys, a0, sigma, Cs = draw_problem(spr, rows, 2, seed=7)
    out = spr.assimilate(ys, a0, sigma)
    check_against_oracle(spr, rows, ys, a0, Cs, out, 'three scales')
    neg = [y.copy() for y in ys]
    for y in neg:
        y[:, 2] = np.where(y[:, 2] == 2, -1.0, y[:, 2])      # -1 wraps to the last feature, as numpy indexing does in predict
    out2 = spr.assimilate(neg, a0, sigma)
    for x, y in zip(out, out2):
        np.testing.assert_array_equal(x, y)
    bad = ys[0].copy()
    bad[0, 2] = 3
    with pytest.raises(IndexError, match='out of bounds'):
        spr.assimilate(bad, a0[0], sigma[0])
    assert spr._engine().assim_calls == 2


def test_single_vector_and_broadcast_prior():
    spr, rows = trained_spr(8)
    ys, a0, sigma, Cs = draw_problem(spr, rows, 3, seed=2)
    one = spr.assimilate(ys[1], a0[1], sigma[1])
    assert one[0].shape == (1, 6) and one[2].shape == (1, 6, 6)
    many = spr.assimilate(ys, a0[1], sigma[1])
    many_f = spr.assimilate(ys, a0[1], prior_factor=Cs[1])
    assert many[0].shape == (3, 6)
    for k in range(3):
        np.testing.assert_array_equal(one[k][0], many[k][1])
    np.testing.assert_allclose(many_f[0], many[0], rtol=0, atol=1e-12 * np.abs(many[0]).max())


def test_two_batches_equal_one_batch():
    """Bayesian consistency: sensors 1..s1, then s1+1..s with the first posterior (Ar, factor) as the prior = all at once"""
    s, s1, r = 11, 4, 6
    spr, rows = trained_spr(s)
    ys, a0, sigma, Cs = draw_problem(spr, rows, 3, seed=3)
    Ar, Ar_std, F = spr.assimilate(ys, a0, sigma)
    info = dict(spr.assimilate_info_)
    first, _ = trained_spr(s1, rows=rows[:s1])
    second, _ = trained_spr(s - s1, rows=rows[s1:])
    A1, _, F1 = first.assimilate([y[:s1] for y in ys], a0, sigma)
    chi2_1, ld_1 = first.assimilate_info_['chi2'], first.assimilate_info_['logdet']
    A2, S2, F2 = second.assimilate([y[s1:] for y in ys], A1, prior_factor=F1)
    Theta = np.asarray(spr.Theta)
    for p, y in enumerate(ys):
        y0, sig0 = scaled(spr, rows, y)
        ref = kalman_oracle(Theta, y0, sig0, a0[p], Cs[p])
        m = 2 * bar_factor(s, r, ref['kappa'])               # two updates, each within the bar of its own exact result
        z = (A2[p] - a0[p]) / sigma[p]
        assert np.linalg.norm(z - ref['z']) <= m * np.linalg.norm(ref['z'])
        assert np.linalg.norm(F2[p] @ F2[p].T - ref['cov']) <= m * np.linalg.norm(ref['cov'])
    np.testing.assert_allclose(A2, Ar, rtol=0, atol=1e-11 * np.abs(Ar).max())
    np.testing.assert_allclose(S2, Ar_std, rtol=1e-11)
    # the innovation statistics of the two steps add up to those of the joint update (chain rule of the evidence)
    np.testing.assert_allclose(chi2_1 + second.assimilate_info_['chi2'], info['chi2'], rtol=1e-9)
    np.testing.assert_allclose(ld_1 + second.assimilate_info_['logdet'], info['logdet'], rtol=1e-9, atol=1e-9)


def test_cov_factor_and_sigma_forms_agree_for_a_diagonal_prior():
    spr, rows = trained_spr(7)
    ys, a0, sigma, Cs = draw_problem(spr, rows, 2, seed=4)
    a = spr.assimilate(ys, a0, sigma)
    b = spr.assimilate(ys, a0, prior_factor=Cs)
    c = spr.assimilate(ys, a0, prior_cov=np.stack([np.diag(sg ** 2) for sg in sigma]))
    assert spr.assimilate_info_['prior'] == 'cov'
    scale = np.abs(a[0]).max()
    for other in (b, c):
        np.testing.assert_allclose(other[0], a[0], rtol=0, atol=1e-11 * scale)
        np.testing.assert_allclose(other[1], a[1], rtol=1e-10)
        np.testing.assert_allclose(np.einsum('pij,pkj->pik', other[2], other[2]), np.einsum('pij,pkj->pik', a[2], a[2]),
                                   rtol=0, atol=1e-10 * np.abs(a[2]).max() ** 2)
    with pytest.raises(ValueError, match='not positive semi-definite'):
        spr.assimilate(ys, a0, prior_cov=-np.eye(6))
    zero = spr.assimilate(ys, a0, prior_cov=np.zeros((6, 6)))
    np.testing.assert_array_equal(zero[0], a0)
    assert not zero[1].any() and not zero[2].any()


def test_exact_properties_of_a_pinned_coefficient():
    spr, rows = trained_spr(9)
    ys, a0, sigma, Cs = draw_problem(spr, rows, 3, seed=6, zero_sigma=(np.array([0, 0, 2]), np.array([1, 4, 3])))
    sigma[1] = 0.0
    Ar, Ar_std, F = spr.assimilate(ys, a0, sigma)
    pinned = sigma == 0
    np.testing.assert_array_equal(Ar[pinned], a0[pinned])
    assert not Ar_std[pinned].any() and not F[pinned].any()
    np.testing.assert_array_equal(Ar[1], a0[1])
    assert not Ar_std[1].any() and not F[1].any()
    assert np.all(Ar[~pinned] != a0[~pinned]) and np.all(Ar_std[~pinned] > 0)
    Cs = np.stack([np.diag(sg) for sg in sigma])
    for p in (0, 2):                                          # the free coefficients still meet the oracle
        y0, sig0 = scaled(spr, rows, ys[p])
        ref = kalman_oracle(np.asarray(spr.Theta), y0, sig0, a0[p], Cs[p])
        m = bar_factor(9, 6, ref['kappa'])
        assert np.linalg.norm(F[p] @ F[p].T - ref['cov']) <= m * np.linalg.norm(ref['cov'])
        assert np.linalg.norm(Ar[p] - ref['a']) <= m * np.linalg.norm(ref['z']) * sigma[p].max() + 4 * EPS * np.linalg.norm(Ar[p])


@pytest.mark.parametrize('s0', [1.0, 30.0, 1e3])
def test_flat_prior_limit_approaches_predict(s0):
    """s >= r: |a - a_ols| <= |a_ols - a0| / (1 + s0^2 lambda_min(Theta^T R^-1 Theta))"""
    spr, rows = trained_spr(10)
    ys, a0, _, _ = draw_problem(spr, rows, 2, seed=8)
    a_ols, _ = spr.predict(ys)
    Ar, _, _ = spr.assimilate(ys, a0, np.full(6, s0))
    Theta = np.asarray(spr.Theta)
    for p, y in enumerate(ys):
        _, sig0 = scaled(spr, rows, y)
        lam = np.linalg.eigvalsh((Theta / sig0[:, None]).T @ (Theta / sig0[:, None]))[0]
        gap = np.linalg.norm(a_ols[p] - a0[p])
        # + the rounding of the two solves: cond(W Theta) eps of predict, kappa(H') eps of assimilate
        slack = 64 * EPS * (1 + s0 ** 2 * np.linalg.eigvalsh((Theta / sig0[:, None]).T @ (Theta / sig0[:, None]))[-1]) * gap
        assert np.linalg.norm(Ar[p] - a_ols[p]) <= gap / (1 + s0 ** 2 * lam) + slack


def test_device_tensors_in_and_out_and_the_field_chain():
    spr, rows = trained_spr(9)
    ys, a0, sigma, Cs = draw_problem(spr, rows, 2, seed=9)
    host = spr.assimilate(ys, a0, sigma)
    dev = spr.assimilate(ys, torch.from_numpy(a0), torch.from_numpy(sigma), to_host=False)
    assert all(isinstance(x, torch.Tensor) for x in dev)
    for h, d in zip(host, dev):
        np.testing.assert_array_equal(h, d.numpy())
    again = spr.assimilate(ys, dev[0], prior_factor=dev[2], to_host=False)        # an earlier posterior as the next prior
    assert tuple(again[2].shape) == (2, 6, 6)
    std = spr.reconstruct_std(factor=dev[2])
    U, scl = np.asarray(spr.Ur), np.asarray(spr.X_scl)[:, 0]
    want = scl[:, None] * np.sqrt(np.einsum('ic,pcd,id->ip', U, np.einsum('pij,pkj->pik', host[2], host[2]), U))
    np.testing.assert_allclose(std, want, rtol=1e-9, atol=1e-12 * want.max())
    empty = spr.assimilate([], np.zeros(6), np.ones(6))
    assert empty[0].shape == (0, 6) and empty[1].shape == (0, 6) and empty[2].shape == (0, 6, 6)
    assert spr.assimilate([], np.zeros(6), prior_factor=np.ones((6, 2)))[2].shape == (0, 6, 2)


def test_refusals_come_before_any_engine_call():
    eng = AssimNumpyEngine()
    spr, rows = trained_spr(9, engine=eng)
    ys, a0, sigma, Cs = draw_problem(spr, rows, 2, seed=1)
    ok = dict(y=ys, prior_mean=a0, prior_sigma=sigma)

    def refused(exc, match, **change):
        kw = dict(ok, **change)
        with pytest.raises(exc, match=match):
            spr.assimilate(kw.pop('y'), kw.pop('prior_mean'), kw.pop('prior_sigma'), **kw)

    fresh = SPR(make_field(), 3, None, engine=eng)
    fresh.fit(select_modes='number', n_modes=6)
    with pytest.raises(AttributeError, match='train'):
        fresh.assimilate(ys, a0, sigma)
    refused(ValueError, 'rows of Theta', y=[y[:5] for y in ys])
    refused(ValueError, 'wrong number of columns', y=[y[:, :2] for y in ys])
    refused(ValueError, 'exactly one of', prior_sigma=None)
    refused(ValueError, 'exactly one of', prior_factor=Cs)
    refused(ValueError, 'exactly one of', prior_factor=Cs, prior_cov=Cs)
    refused(ValueError, r'prior_mean must have shape \(2, 6\) or \(6,\)', prior_mean=a0[:, :5])
    refused(ValueError, r'prior_mean must have shape \(2, 6\) or \(6,\)', prior_mean=np.zeros((3, 6)))
    refused(ValueError, r'prior_sigma must have shape \(2, 6\) or \(6,\)', prior_sigma=np.ones((6, 2)))
    refused(ValueError, r'prior_factor must have shape \(2, 6, q\) or \(6, q\) with 1 <= q <= 6', prior_sigma=None,
            prior_factor=np.ones((6, 7)))
    refused(ValueError, r'prior_factor must have shape', prior_sigma=None, prior_factor=np.ones((2, 5, 3)))
    refused(ValueError, r'prior_factor must have shape', prior_sigma=None, prior_factor=np.ones((6, 0)))
    refused(ValueError, r'prior_cov must have shape \(2, 6, 6\) or \(6, 6\)', prior_sigma=None, prior_cov=np.ones((2, 6, 5)))
    for v in (-1.0, np.nan, np.inf):
        bad = sigma.copy()
        bad[1, 2] = v
        refused(ValueError, 'finite and >= 0', prior_sigma=bad)
        refused(ValueError, 'finite and >= 0', prior_sigma=torch.from_numpy(bad))
    for v in (0.0, np.nan, np.inf):
        bad = [y.copy() for y in ys]
        bad[1][3, 1] = v
        refused(ValueError, 'sensor uncertainty', y=bad)
    refused(ValueError, 'sensor uncertainty', y=[np.concatenate([y[:, :1], 0 * y[:, 1:2], y[:, 2:]], axis=1) for y in ys])
    spr.method = 'COLS'
    refused(NotImplementedError, 'COLS')
    spr.method = 'other'
    refused(NotImplementedError, 'not been')
    spr.method = 'OLS'
    assert eng.assim_calls == 0
    spr.assimilate(ys, a0, sigma)
    assert eng.assim_calls == 1


def test_more_modes_than_the_kernel_takes_is_refused():
    eng = AssimNumpyEngine()
    rng = np.random.default_rng(0)
    X = rng.standard_normal((300, 140))
    spr = SPR(X, 1, None, engine=eng)
    spr.fit(select_modes='number', n_modes=129)
    C = np.zeros((130, 300))
    C[np.arange(130), np.arange(130)] = 1.0
    spr.train(C)
    y = np.stack([rng.standard_normal(130), np.ones(130), np.zeros(130)], axis=1)
    with pytest.raises(NotImplementedError, match='up to 128 modes'):
        spr.assimilate(y, np.zeros(129), np.ones(129))
    assert eng.assim_calls == 0


# ------------------------------------------------------------------------------------------------ two ranks over gloo
def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from openmeasure_amd.sparse_sensing import SPR, RowShard
        from tests.test_assimilate_host import AssimNumpyEngine, draw_problem, make_field, trained_spr
        X = make_field()
        n = X.shape[0]
        cuts = [0, 50, n]                                      # cut by hand inside a feature (features of 40 rows)
        row0, n_loc = cuts[rank], cuts[rank + 1] - cuts[rank]
        spr = SPR(np.ascontiguousarray(X[row0:row0 + n_loc]), 3, None, shard=RowShard(row0, n), engine=AssimNumpyEngine())
        spr.fit(select_modes='number', n_modes=6)
        rows = np.sort(np.random.default_rng(1).choice(n, size=9, replace=False))
        C = np.zeros((9, n))
        C[np.arange(9), rows] = 1.0
        spr.train(C)
        whole, rows_w = trained_spr(9)                         # the unsharded object draws the problem: the same on both ranks
        ys, a0, sigma, Cs = draw_problem(whole, rows_w, 2, seed=11)
        calls = []
        ag, ar = spr._all_gather, spr._all_reduce
        spr._all_gather = lambda t: (calls.append('gather'), ag(t))[1]
        spr._all_reduce = lambda t: (calls.append('reduce'), ar(t))[1]
        Ar, As, F = spr.assimilate(ys, a0, sigma)
        Ar2, As2, F2 = spr.assimilate(ys, a0, prior_factor=Cs)
        np.savez(os.path.join(out_dir, f'rank{rank}.npz'), Ar=Ar, As=As, F=F, Ar2=Ar2, As2=As2, F2=F2, calls=len(calls),
                 chi2=spr.assimilate_info_['chi2'])
    finally:
        dist.destroy_process_group()


def test_two_ranks_return_identical_arrays_without_a_collective(tmp_path):
    import torch.multiprocessing as mp
    from tests.test_cols_host import _free_port
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    got = [np.load(tmp_path / f'rank{q}.npz') for q in range(2)]
    for k in ('Ar', 'As', 'F', 'Ar2', 'As2', 'F2', 'chi2'):
        np.testing.assert_array_equal(got[0][k], got[1][k])
    assert got[0]['calls'] == 0 and got[1]['calls'] == 0
