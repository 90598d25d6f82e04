"""The kernels of csrc/cokriging.hip on the GPU against the NumPy oracle of tests/test_cokriging_host.py, at the kernel's
edges rather than the workload's (the rationale of tests/test_gpr_gpu.py): the block row of 16, the LDS chunk of 32 contraction
rows and the 256 threads that each own one column -- n in {P + 1, 37, 64, 65, 130, 257} -- with d in {1, 3}, r in {1, 5}, both trends,
with and without the rho column, Y with a row stride.

THE BAR of the factor-only tests (written before the first GPU run).  rel = c n eps kappa_2(R), eps = 2^-53, c = 16 + d:
* 12 = 3 x 4 for the four explicitly formed factors (Cholesky factor, its inverse, X^T X, and a product with R^-1: R^-1 F or
  R^-1 res), each with a backward error of about 3 n eps |R| (Higham, Accuracy and Stability, Thm 10.4): the count of
  tests/test_gpr_gpu.py, the code is shared (gp_core.hpp).
* 4 + d for forming R from quantities that carry RELATIVE errors only: pow (2 ulp of the device library), exp (1), the nugget's
  addition (1), and per coordinate the product theta u and the fma -- the kernel subtracts BEFORE it scales, so u = x_ic - x_jc is
  one rounding of exact inputs and s carries (d + 3) eps s; |d exp(-s)| <= (d + 3) eps s exp(-s) < (d + 3) eps / e per entry,
  |dR|_2 <= (4 + d) n eps |R|_2 since |R|_2 >= 1.
A backward error of rel / kappa in R moves R^-1 by rel |R^-1|_2; what follows is first-order propagation of that, with
sR = |R^-1|_2 and, where the trend solve enters, another factor kappa_2(G) (the sums that form G = F^T (R^-1 F) cancel by up to
kappa(R): |dG| / |G| ~ n eps kappa(R), and the P x P solve multiplies it by kappa(G)): relG = rel kappa_2(G).
    R^-1:        rel sR                               R^-1 F[:, c]:  rel sR |F[:, c]|_2
    G^-1:        relG |G^-1|_2
    beta:        b_beta  = relG |beta|_2 + rel sqrt(|G^-1|_2 / sR) |gamma|_2
                 (d beta = -G^-1 F^T R^-1 E gamma and |G^-1 F^T R^-1|_2 <= sqrt(|G^-1|_2 |R^-1|_2))
    gamma:       b_gamma = rel sR |res|_2 + |R^-1 F|_2 b_beta
    sigma2:      b_s2    = (|gamma|_2 |F|_2 b_beta + |res|_2 b_gamma) / (n - P)
    loss:        ((n - P) b_s2 / sigma2 + rel (n + sum |log pivots|)) / n          (d log det (R + E) = tr R^-1 E <= n rel)
    grad_c:      ln10 / n [ (rel sR + 2 |gamma|_inf b_gamma / sigma2 + |gamma|_inf^2 b_s2 / sigma2^2) sum T_c + rel sum |W| T_c ],
                 T_c = theta_c u_c^2 exp(-s) >= 0.
The reference values are the oracle in np.longdouble; kappa is taken from its R and G.  Inputs are chosen so that rel < 1e-8
(asserted): noisy targets, nugget 1e-3, theta between 1 and 3.2, points spread by (n / 16)^(1/d) so that their density, and with it
kappa(R), does not grow with n.

Trajectory bar: that of tests/test_gpr_gpu.py over d parameters -- a gradient error dg_c changes Adam's step by at most
2 lr dg_c / sqrt(v^_c); with dg_c the gradient's bar at evaluation i, the bar of parameter c at evaluation j is
sum_{i < j} 2 x 2 lr max_{i' <= i} dg_c / sqrt(v^_c,i) + 8 eps (|v_c| + lr) j.  The clip is a contraction: it keeps the bar.
These are worst-case bounds chained through the trend solve and they come out loose (the gradient's by ten orders on the
MI355X, the trajectory's with it): what they catch is a wrong term, a wrong index, a missed tile -- errors of order one.  The
sharp check is test_training_to_convergence, whose bar is measured.

Predict bars (predict_bars()), the same propagation with r* carrying (d + 3) eps / e per entry, |dr*|_2 <= rel:
    mean:  |f*|_2 b_beta + |r*|_2 b_gamma + rel (|f*|.|beta| + (|r*|_2 + 1) |gamma|_2)
    mse:   b_s2 Q + sigma2 (dq1 + dq2 + rel Q),   Q = 1 + |r*|_2^2 sR + |u|_2^2 |G^-1|_2,
           dq1 = rel sR (|r*|_2^2 + 2 |r*|_2),   du = rel (sR |F|_2 |r*|_2 + |R^-1 F|_2),   dq2 = 2 |u|_2 |G^-1|_2 du + relG |u|_2^2 |G^-1|_2."""
import numpy as np
import pytest

from openmeasure_amd.cokriging import CoKriging
from tests.test_cokriging_host import (CkNumpyEngine, ck_case, ck_loss_grad, ck_predict, ck_sqdist, ck_train, ck_trend,
                                       two_mesh_case)

pytestmark = pytest.mark.gpu
LD = np.longdouble
EPS = 2.0 ** -53
F64 = lambda a: np.asarray(a, dtype=np.float64)
NUGGET = 1e-3
V_LO, V_HI = -5.0, float(np.log10(50.0))


@pytest.fixture(scope='module')
def eng():
    from openmeasure_amd.engine import HipEngine
    return HipEngine('cuda:0')


def strided(eng, Y, pad=3):
    buf = np.zeros((Y.shape[0], Y.shape[1] + pad))
    buf[:, :Y.shape[1]] = Y
    t = eng.to_device(buf)[:, :Y.shape[1]]
    assert t.stride(0) == Y.shape[1] + pad
    return t


def spread(n, d):
    return max(1.0, n / 16.0) ** (1.0 / d)


def vset(q, d):
    """log10 theta of model q: theta_c = (1 + c / 2) (1 + 0.3 (q mod 3)), between 1 and 3.2"""
    return np.log10(np.array([(1.0 + 0.5 * c) * (1.0 + 0.3 * (q % 3)) for c in range(d)]))


def n_trend(d, regr, with_rho):
    return (1 if with_rho else 0) + 1 + (d if regr == 'linear' else 0)


def bars(ev, n, d):
    """absolute bars of every output of an evaluation (module docstring), from an oracle evaluation -> dict, rel, relG"""
    R, G, F = F64(ev['R']), F64(ev['G']), F64(ev['F'])
    P = F.shape[1]
    rel = (16 + d) * n * EPS * np.linalg.cond(R)
    relG = rel * np.linalg.cond(G)
    sR, sG = np.linalg.norm(F64(ev['Rinv']), 2), np.linalg.norm(F64(ev['Ginv']), 2)
    gam, res, beta, s2 = F64(ev['gamma']), F64(ev['res']), F64(ev['beta']), float(ev['sigma2'])
    gn, rn, ginf = np.linalg.norm(gam), np.linalg.norm(res), np.max(np.abs(gam))
    b_beta = relG * np.linalg.norm(beta) + rel * np.sqrt(sG / sR) * gn
    b_gamma = rel * sR * rn + np.linalg.norm(F64(ev['RinvF']), 2) * b_beta
    b_s2 = (gn * np.linalg.norm(F, 2) * b_beta + rn * b_gamma) / (n - P)
    logsum = np.sum(np.abs(F64(ev['logdiag']))) if ev['logdiag'] is not None else n * abs(np.log(np.linalg.cond(R)))
    b_loss = ((n - P) * b_s2 / s2 + rel * (n + logsum)) / n
    dw = rel * sR + 2 * ginf * b_gamma / s2 + ginf * ginf * b_s2 / (s2 * s2)
    T = F64(ev['tu2']) * F64(ev['Rc'])
    b_grad = np.array([np.log(10.0) / n * (dw * np.sum(T[c]) + rel * np.sum(np.abs(F64(ev['W'])) * T[c])) for c in range(d)])
    out = dict(Rinv=rel * sR, RinvF=rel * sR * np.linalg.norm(F, axis=0), Ginv=relG * sG, beta=b_beta, gamma=b_gamma, sigma2=b_s2,
               loss=b_loss, grad=b_grad)
    return out, rel, relG


FACTOR_N = [('P+1', 5), (37, 1), (64, 5), (65, 1), (130, 5), (257, 1)]                     # n and r, alternating
FACTOR_CASES = [(n, r, d, regr, with_rho) for n, r in FACTOR_N for d in (1, 3) for regr in ('constant', 'linear')
                for with_rho in (False, True)]


@pytest.mark.parametrize('n,r,d,regr,with_rho', FACTOR_CASES)
def test_factor_only(eng, n, r, d, regr, with_rho):
    """max_iter = 0 at fixed v (model q at vset(q, d); with r = 1, q = n + d): R^-1, R^-1 F, G^-1, beta, gamma, sigma2, the loss
    and every gradient component against the longdouble oracle at the bars of the module docstring."""
    P = n_trend(d, regr, with_rho)
    n = P + 1 if n == 'P+1' else n
    X, Y, rho = ck_case(n, d, r, seed=n + d, noise=0.3, spread=spread(n, d))
    vs = np.array([vset(q if r > 1 else n + d, d) for q in range(r)])
    v, fit, info, tr = eng.ck_train(eng.to_device(X), strided(eng, Y), strided(eng, rho) if with_rho else None, regr,
                                    eng.to_device(vs), NUGGET, V_LO, V_HI, 0.1, 0, 0.0)
    v, info = eng.to_host(v), eng.to_host(info)
    fit = {k: eng.to_host(t) for k, t in fit.items()}
    assert tr is None and np.array_equal(v, vs) and info.shape == (r, 4 + d)
    assert np.all(info[:, 0] == 0) and np.all(info[:, 3] == 0)
    assert fit['RinvF'].shape == (r, n, P) and fit['Ginv'].shape == (r, P, P) and fit['beta'].shape == (r, P)
    for q in range(r):
        ev = ck_loss_grad(X, Y[:, q], vs[q], regr, rho[:, q] if with_rho else None, NUGGET, dtype=LD)
        bar, rel, relG = bars(ev, n, d)
        assert rel < 1e-8, rel
        errs = {k: np.max(np.abs(fit[k][q] - ev[k]), axis=0 if k == 'RinvF' else None) for k in ('Rinv', 'RinvF', 'Ginv', 'beta', 'gamma')}
        errs.update(sigma2=abs(fit['sigma2'][q] - ev['sigma2']), loss=abs(info[q, 1] - ev['loss']), grad=np.abs(info[q, 4:] - ev['grad']))
        print(f'factor n={n} d={d} {regr} rho={with_rho} model {q}: rel {rel:.2e} relG {relG:.2e} errors / bar ' +
              ' '.join(f'{k} {float(np.max(F64(e) / np.maximum(bar[k], 1e-300))):.2e}' for k, e in errs.items()))
        assert np.array_equal(fit['Rinv'][q], fit['Rinv'][q].T)          # both halves add the same products in the same order
        assert np.array_equal(fit['Ginv'][q], fit['Ginv'][q].T)
        for k, e in errs.items():
            assert np.all(F64(e) <= bar[k]), (k, F64(e), bar[k])


TRAJ_CASES = [(37, 1, 'linear', False, V_HI), (65, 3, 'linear', True, 0.0), (130, 3, 'constant', True, V_HI)]


@pytest.mark.parametrize('n,d,regr,with_rho,v_hi', TRAJ_CASES)
def test_trajectory_of_25_evaluations(eng, n, d, regr, with_rho, v_hi):
    """The trace of 25 evaluations (tol = 0) from theta0 = 0.5, parameter by parameter, against the float64 oracle at the
    trajectory bar of the module docstring.  With v_hi = 0 (n = 65) two coordinates of model 2 reach the bound at the fifth
    evaluation and stay there for the other 21 while the third moves on: where the oracle's coordinate sits on the bound, the
    kernel's sits on it exactly.  In models 0 and 1 EVERY coordinate reaches the bound: the next loss repeats bit for bit,
    e = 0 <= tol = 0, and they stop after 6 evaluations -- on the device as in the oracle (the counts are compared)."""
    r, n_it, lr = 3, 25, 0.1
    X, Y, rho = ck_case(n, d, r, seed=10 + n, noise=0.3, spread=spread(n, d))
    v0 = np.full((r, d), np.log10(0.5))
    v, fit, info, tr = eng.ck_train(eng.to_device(X), strided(eng, Y), strided(eng, rho) if with_rho else None, regr,
                                    eng.to_device(v0), NUGGET, V_LO, v_hi, lr, n_it, 0.0, trace=True)
    tr, info, v = eng.to_host(tr), eng.to_host(info), eng.to_host(v)
    assert tr.shape == (r, n_it, 1 + d) and np.all(info[:, 3] == 0)
    clipped = 0
    for q in range(r):
        rq = rho[:, q] if with_rho else None
        t = ck_train(X, Y[:, q], regr, rq, v0[q], NUGGET, V_LO, v_hi, lr, n_it, 0.0)
        n_q = t['iterations']
        assert info[q, 0] == n_q and (n_q == n_it or v_hi == 0.0)
        bar, dg_max, m2, b2t, worst = np.zeros(d), np.zeros(d), np.zeros(d), 1.0, 0.0
        for j in range(n_q):
            p = t['trace'][j, 1:]
            ev = ck_loss_grad(X, Y[:, q], p, regr, rq, NUGGET)
            b, rel, _ = bars(ev, n, d)
            dp = np.abs(tr[q, j, 1:] - p)
            dl = abs(tr[q, j, 0] - t['trace'][j, 0])
            bar_j = bar + 8 * EPS * (np.abs(p) + lr) * j
            worst = max(worst, float(np.max(dp / np.maximum(bar_j, 1e-300))) if j else 0.0)
            assert np.all(dp <= bar_j), (q, j, dp, bar_j)
            assert dl <= b['loss'] + np.sum(np.abs(ev['grad']) * bar_j), (q, j, dl)
            on = (p == v_hi)
            clipped += int(on.sum())
            assert np.all(tr[q, j, 1:][on] == v_hi) or j == 0
            dg_max = np.maximum(dg_max, b['grad'])
            b2t *= 0.999
            m2 = 0.999 * m2 + 0.001 * ev['grad'] ** 2
            bar = bar + 2 * 2 * lr * dg_max / np.sqrt(m2 / (1 - b2t))
        print(f'trajectory n={n} d={d} model {q}: {n_q} evaluations, max |d v| {np.max(np.abs(tr[q, :n_q, 1:] - t["trace"][:, 1:])):.2e} final bar {bar.tolist()} '
              f'worst ratio {worst:.2e}; last v {t["trace"][-1, 1:].tolist()}')
        assert np.all(np.abs(v[q] - t['v']) <= bar + 8 * EPS * (np.abs(t['v']) + lr) * n_q)
        assert info[q, 1] == tr[q, n_q - 1, 0]                   # the info row holds the last evaluation with a step
        assert np.all(tr[q, :, 1:] <= v_hi) and np.all(tr[q, :, 1:] >= V_LO)
    if v_hi == 0.0:
        assert clipped >= 30                                     # the case is there for the clip: it must have happened


CONV_BAR_37, CONV_BAR_130 = 1.1e-12, 1.9e-12
CONV_CASES = [(37, 1, 5, CONV_BAR_37), (130, 3, 6, CONV_BAR_130)]


@pytest.mark.parametrize('n,d,seed,bar', CONV_CASES)
def test_training_to_convergence(eng, n, d, seed, bar):
    """Default training (theta0 0.5, bounds 1e-5 .. 50, lr 0.1, max_iter 1000, tol 1e-6; linear trend) of 3 models without and 3
    with the rho column on ck_case(n, d, 3, seed, noise=0.3) with the nugget 1e-3 of this file's noisy targets.  The oracle stops
    after 95/102/84 and 113/107/89 (n = 37), 91/131/85 and 142/102/149 (n = 130) evaluations, and its last two e lie more than
    1 % away from tol in every model (checked on the CPU, asserted again here), so the evaluation count must be equal.  The bar
    on the final v is MEASURED on the CPU: ten times the larger of the final differences between the float64 oracle and (a) the
    float64 oracle with R^-1 and log det from LU (route='inv'), (b) the longdouble oracle, over the six models --
    n = 37: (a) 1.08e-13, (b) 7.25e-14 -> 1.1e-12;  n = 130: (a) 1.26e-13, (b) 1.86e-13 -> 1.9e-12."""
    r, tol = 3, 1e-6
    X, Y, rho = ck_case(n, d, r, seed=seed, noise=0.3, spread=spread(n, d))
    v0 = np.full((r, d), np.log10(0.5))
    out = {}
    for with_rho in (False, True):
        v, fit, info, _ = eng.ck_train(eng.to_device(X), strided(eng, Y), strided(eng, rho) if with_rho else None, 'linear',
                                       eng.to_device(v0), NUGGET, V_LO, V_HI, 0.1, 1000, tol)
        out[with_rho] = eng.to_host(v), eng.to_host(info)
    ts = {(w, q): ck_train(X, Y[:, q], 'linear', rho[:, q] if w else None, nugget=NUGGET) for w in (False, True) for q in range(r)}
    for (w, q), t in ts.items():
        v, info = out[w]
        assert abs(t['es'][-1] / tol - 1) > 0.01 and abs(t['es'][-2] / tol - 1) > 0.01 and t['iterations'] < 1000
        print(f'training n={n} rho={w} model {q}: evaluations {int(info[q, 0])} / {t["iterations"]}, e {info[q, 2]:.3e} / {float(t["e"]):.3e}, '
              f'max |d v| {np.max(np.abs(v[q] - t["v"])):.2e} (bar {bar:.1e})')
    for (w, q), t in ts.items():
        v, info = out[w]
        assert info[q, 3] == 0 and int(info[q, 0]) == t['iterations']
        assert np.max(np.abs(v[q] - t['v'])) <= bar


def predict_bars(ev, fs, rs, n, d):
    """absolute bars of mean and mse_own at test points with trend rows fs and correlations rs (module docstring)"""
    b, rel, relG = bars(ev, n, d)
    sR, sG = np.linalg.norm(F64(ev['Rinv']), 2), np.linalg.norm(F64(ev['Ginv']), 2)
    rn, fn = np.linalg.norm(rs, axis=1), np.linalg.norm(fs, axis=1)
    un = np.linalg.norm(rs @ F64(ev['RinvF']) - fs, axis=1)
    s2, gn, RFn = float(ev['sigma2']), np.linalg.norm(F64(ev['gamma'])), np.linalg.norm(F64(ev['RinvF']), 2)
    b_mean = fn * b['beta'] + rn * b['gamma'] + rel * (np.abs(fs) @ np.abs(F64(ev['beta'])) + (rn + 1) * gn)
    dq1 = rel * sR * (rn * rn + 2 * rn)
    du = rel * (sR * np.linalg.norm(F64(ev['F']), 2) * rn + RFn)
    dq2 = 2 * un * sG * du + un * un * relG * sG
    quad = 1 + rn * rn * sR + un * un * sG
    b_mse = b['sigma2'] * quad + s2 * (dq1 + dq2 + rel * quad)
    return b_mean, b_mse, rel


@pytest.mark.parametrize('n,d,n_p,regr,with_rho', [(37, 1, 1, 'linear', False), (65, 3, 70, 'linear', True), (6, 3, 70, 'linear', True),
                                                   (300, 3, 70, 'constant', True), (130, 1, 9, 'constant', False)])
def test_predict_against_the_closed_form(eng, n, d, n_p, regr, with_rho):
    """mean and mse_own against longdouble at the predict bars.  Row 0 of Xstar is a training point: the mean is its target to
    the nugget (|mean - y| <= nugget |gamma_i| + bar) and mse_own <= 2 nugget sigma2 + bar.  With n_p > 1, row 1 lies 1000
    units away: r* = 0 exactly, mean = f*.beta and mse_own = sigma2 (1 + f*^T G^-1 f*) to rounding."""
    r = 3
    X, Y, rho = ck_case(n, d, r, seed=20 + n, noise=0.3, spread=spread(n, d))
    vs = np.array([vset(q, d) for q in range(r)])
    rng = np.random.default_rng(n)
    Xs = rng.standard_normal((n_p, d)) * 1.5 * spread(n, d)
    i0 = min(3, n - 1)
    Xs[0] = X[i0]
    if n_p > 1:
        Xs[1] = X.mean(axis=0) + 1000.0
    rs_star = rng.standard_normal((n_p, r))
    rs_star[0] = rho[i0]
    X_d = eng.to_device(X)
    v, fit, info, _ = eng.ck_train(X_d, eng.to_device(Y), eng.to_device(rho) if with_rho else None, regr, eng.to_device(vs), NUGGET,
                                   V_LO, V_HI, 0.1, 0, 0.0)
    assert np.all(eng.to_host(info)[:, 3] == 0)
    mean, mse = eng.ck_predict(X_d, eng.to_device(Xs), strided(eng, rs_star) if with_rho else None, regr, v, fit)
    mean, mse = eng.to_host(mean), eng.to_host(mse)
    assert mean.shape == mse.shape == (n_p, r)
    worst = 0.0
    for q in range(r):
        rq, rsq = (rho[:, q], rs_star[:, q]) if with_rho else (None, None)
        ev = ck_loss_grad(X, Y[:, q], vs[q], regr, rq, NUGGET, dtype=LD)
        want_m, want_s = ck_predict(X, Xs, vs[q], ev, regr, rsq)
        fs = ck_trend(Xs, regr, rsq)
        rs = np.exp(-ck_sqdist(Xs, X, 10.0 ** vs[q])[0])
        b_mean, b_mse, rel = predict_bars(ev, fs, rs, n, d)
        em, es = np.abs(mean[:, q] - F64(want_m)), np.abs(mse[:, q] - F64(want_s))
        worst = max(worst, float(np.max(em / b_mean)), float(np.max(es / b_mse)))
        assert np.all(em <= b_mean) and np.all(es <= b_mse), (q, em / b_mean, es / b_mse)
        assert np.all(mse[:, q] >= 0)
        s2, gam = float(ev['sigma2']), F64(ev['gamma'])
        assert abs(mean[0, q] - Y[i0, q]) <= NUGGET * abs(gam[i0]) + b_mean[0]                # a training point
        assert mse[0, q] <= 2 * NUGGET * s2 + b_mse[0]
        if n_p > 1:
            fb = float(fs[1] @ F64(ev['beta']))
            assert rs[1].max() == 0.0
            assert abs(mean[1, q] - fb) <= b_mean[1]
            far = s2 * (1 + fs[1] @ F64(ev['Ginv']) @ fs[1])
            assert abs(mse[1, q] - far) <= b_mse[1]
    print(f'predict n={n} d={d} n_p={n_p} {regr} rho={with_rho}: worst error / bar {worst:.2e}')


def test_two_runs_agree_bit_for_bit(eng):
    n, d, r = 130, 3, 5
    X, Y, rho = ck_case(n, d, r, seed=7, noise=0.3, spread=spread(n, d))
    Xs = np.random.default_rng(1).standard_normal((70, d)) * spread(n, d)
    runs = []
    for _ in range(2):
        X_d = eng.to_device(X)
        v, fit, info, tr = eng.ck_train(X_d, strided(eng, Y), strided(eng, rho), 'linear', eng.to_device(np.full((r, d), np.log10(0.5))),
                                        NUGGET, V_LO, V_HI, 0.1, 30, 1e-6, trace=True)
        mean, mse = eng.ck_predict(X_d, eng.to_device(Xs), eng.to_device(Xs @ np.ones((d, r))), 'linear', v, fit)
        runs.append([eng.to_host(t) for t in (v, *[fit[k] for k in eng.CK_FIT_KEYS], info, tr, mean, mse)])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    assert all(np.array_equal(K, K.T) for K in runs[0][1])


def test_a_pivot_that_is_not_finite_stops_its_model_only(eng):
    """v = NaN in model 0 makes its first pivot NaN: status 2 for that model, v left as given, no evaluation counted; model 1
    trains as if alone (bit for bit: no workgroup reads another's data)."""
    X, Y, rho = ck_case(37, 2, 2, seed=3, noise=0.3)
    vs = np.array([[np.nan, 0.0], [np.log10(0.5)] * 2])
    args = (NUGGET, V_LO, V_HI, 0.1, 5, 0.0)
    v, fit, info, _ = eng.ck_train(eng.to_device(X), eng.to_device(Y), eng.to_device(rho), 'linear', eng.to_device(vs), *args)
    info, v = eng.to_host(info), eng.to_host(v)
    assert info[0, 3] == 2 and info[0, 0] == 0 and np.array_equal(v[0], vs[0], equal_nan=True)
    v1, fit1, info1, _ = eng.ck_train(eng.to_device(X), eng.to_device(Y[:, 1:]), eng.to_device(rho[:, 1:]), 'linear', eng.to_device(vs[1:]), *args)
    assert info[1, 3] == 0 and info[1, 0] == 5 and np.array_equal(v[1], eng.to_host(v1)[0])
    assert np.array_equal(info[1], eng.to_host(info1)[0]) and np.array_equal(eng.to_host(fit['Rinv'])[1], eng.to_host(fit1['Rinv'])[0])
    t = ck_train(X, Y[:, 1], 'linear', rho[:, 1], vs[1], *args)
    assert np.allclose(v[1], t['v'], rtol=0, atol=1e-11)


def test_end_to_end_against_the_oracle_driven_double(eng):
    """The public class on the HIP engine against the same class over the oracle-driven engine double, with max_iter = 60 and
    tol = 0 per level, LF on 80 rows and HF on 134.  Z_pred, Z_mse, Y_pred and Y_var are held to E2E_BAR kappa_max relative to
    their largest entry, kappa_max the largest condition number of a level's R at the trained
    theta; E2E_BAR is the convergence bar of test_training_to_convergence (the larger of its two cases).  A POD mode's sign is
    the eigensolver's: the scores are compared after the sign of the double's mode is matched.
    thetaL = 0.05 keeps the 8-point HF level a well-posed case: with the default 1e-5 its theta runs to the bound within the 60
    steps, R tends to the all-ones matrix, sigma2 grows to 1e4 and the MSE is a difference of numbers that much larger -- on the
    CPU two factorisation routes of the ORACLE (Cholesky, LU) then differ by 2.3e-4 in Z_mse, six times this bar (and so did
    the kernel, 2.4e-4), against 2.3e-7 at thetaL = 0.05, a 150th of it (measured on the CPU).  With that bound both
    coordinates of LF dimension 0 (nearly linear in the parameters) arrive on it at the 12th evaluation, 0.02 and 0.07 beyond
    it before the clip; the loss then repeats bit for bit, e = 0 <= tol, and that model stops after 13 evaluations in the oracle
    and on the device alike; the other five run all 60.  The counts are compared."""
    args, _ = two_mesh_case()
    X_test = np.array([[0.1, -0.3], [0.7, 0.6], args['X_train_l'][2]])
    out = []
    for e in (eng, CkNumpyEngine()):
        ck = CoKriging(**args, engine=e)
        ck.manifold_alignment(select_modes='number', n_modes_hf=3, n_modes_lf=3)
        ck.max_iter, ck.tol, ck.nugget, ck.thetaL = 60, 0.0, 1e-6, 0.05
        ck.fit()
        Z_pred, Z_mse = ck.predict_latent(X_test)
        Y_pred, Y_var = ck.predict(X_test)
        out.append((ck, Z_pred, Z_mse, Y_pred, Y_var))
    (g, *dev), (h, *ref) = out
    assert np.array_equal(h.cokriging_info_['iterations'][0], [13, 60, 60]) and np.array_equal(h.cokriging_info_['iterations'][1], [60, 60, 60])
    assert all(np.array_equal(g.cokriging_info_['iterations'][lev], h.cokriging_info_['iterations'][lev]) for lev in (0, 1))
    assert g.rom_lf.X.shape == (80, 22) and g.rom_hf.X.shape == (134, 8) and dev[2].shape == (134, 3)
    sign = np.sign(np.sum(g.Zr_hf * h.Zr_hf, axis=1))
    X = np.concatenate([args['X_train_u'], args['X_train_l']])
    Xn = (X - h.X_mean) / h.X_std
    th = h.cokriging_info_['theta']
    cond = lambda Z, theta: np.linalg.cond(np.exp(-ck_sqdist(Z, Z, theta)[0]) + 1e-6 * np.eye(len(Z)))
    kappa = max(max(cond(Xn, th[0][k]), cond(Xn[14:], th[1][k])) for k in range(3))
    tol = max(CONV_BAR_37, CONV_BAR_130) * kappa
    dev[0] = dev[0] * sign[:, None]
    names = ('Z_pred', 'Z_mse', 'Y_pred', 'Y_var')
    for name, a, b in zip(names, dev, ref):
        err = np.max(np.abs(a - b)) / np.max(np.abs(b))
        print(f'end to end {name}: relative error {err:.2e} (bar {tol:.2e}, kappa {kappa:.2e})')
    for name, a, b in zip(names, dev, ref):
        assert a.shape == b.shape and np.max(np.abs(a - b)) <= tol * np.max(np.abs(b)), name
    # the device tensors of predict_latent(to_host=False) go straight into reconstruct
    Zd, Md = g.predict_latent(X_test, to_host=False)
    assert Zd.is_cuda and np.array_equal(g.rom_hf.reconstruct(Zd.T.contiguous()), dev[2])
    assert np.array_equal(g.rom_hf.reconstruct_std(Md.T.sqrt().contiguous()) ** 2, dev[3]) and g.Ur_hf.is_cuda
