"""GPR with a noise per point on the CPU: the NumPy oracle of the model (gp2_loss_grad_noise, gp2_train_noise -- what
spr_gp_train_noise_f64 of csrc/gp.hip is held to in tests/test_gpr_noise_gpu.py), its gradient against central differences, its
reduction to the oracle of tests/test_gpr_ard_host.py, the public ``GPR.update(fixed_noise=True / retrain=True)`` over a NumPy
double of the engine call, and the refusals of the C entry point.

The model (openmeasure_amd/gpr.py): that of tests/test_gpr_ard_host.py for flags 0..3 with, per mode q over the m points,
n_i = w_i s2 + V[i, q], K = o k(t) + diag(n), the same loss, and d loss / d raw_n = sigmoid(raw_n) sum_i w_i (K^-1_ii - alpha_i^2)
/ 2m (d n_i / d raw_n = w_i sigmoid(raw_n)); every other gradient component is unchanged in form.  w = 1, V = 0 is the
homoscedastic model, and the oracle then performs the same floating-point operations as gp2_loss_grad.

Central differences in longdouble with h = 1e-5, as in tests/test_gpr_ard_host.py: truncation ~ 1e-11, rounding ~ 1e-14, the check
asks for 1e-7 max(1, |g|)."""
import pickle

import numpy as np
import pytest
import torch

from openmeasure_amd import _lib
from openmeasure_amd.gpr import GPR, GPKernel, GPRecord, KERNELS
from tests.test_gpr_ard_host import Gp2NumpyEngine, fitted2, gp2_loss_grad, gp2_predict, gp2_train, layout, scaled_t, split, widen
from tests.test_gpr_host import (chol_lower, field_case, gp_case, gp_distance, gp_kernel, gp_predict, sigmoid, softplus,
                                 tri_inv_lower)

LD = np.longdouble
LOG_2PI = np.log(2.0 * np.pi)


# ------------------------------------------------------------------------------------------------ the oracle
def gp2_loss_grad_noise(P0, y, raw, kernel, flags, w, v, dtype=np.float64, route='chol'):
    """gp2_loss_grad with the noise n = w s2 + v per point (w, v of shape (m,)) -> its dict plus n.  route 'chol': Cholesky factor,
    its inverse X, K^-1 = X^T X; 'inv': numpy.linalg.inv and slogdet (LU; float64 only) -- a different route to the same numbers."""
    T = np.dtype(dtype).type
    P0, y, raw = np.asarray(P0, dtype=dtype), np.asarray(y, dtype=dtype), np.asarray(raw, dtype=dtype)
    w, v = np.asarray(w, dtype=dtype), np.asarray(v, dtype=dtype)
    m, d = P0.shape
    assert w.shape == v.shape == (m,)
    L, S, n_par = layout(d, flags)
    ell, o, s2, mu = split(raw, d, flags)
    t, u2 = scaled_t(P0 / ell, P0 / ell)
    k, dk = gp_kernel(kernel, t)
    n = w * s2 + v
    K = o * k + np.diag(n)
    if route == 'chol':
        Lc = np.linalg.cholesky(K) if dtype == np.float64 else chol_lower(K)
        X = tri_inv_lower(Lc)
        Kinv = X.T @ X
        logdiag = 2 * np.log(np.diag(Lc))
        logdet = np.sum(logdiag)
    else:
        Kinv, logdiag, logdet = np.linalg.inv(K), None, np.linalg.slogdet(K)[1]
    res = y - mu
    alpha = Kinv @ res
    loss = (res @ alpha / 2 + logdet / 2 + m * T(LOG_2PI) / 2) / m
    W = Kinv - np.outer(alpha, alpha)
    if flags & 1:
        gl = [sigmoid(raw[c]) * (o * np.sum(W * dk * u2[c] / (t * t)) / ell[c]) / (2 * m) for c in range(d)]
    else:
        gl = [sigmoid(raw[0]) * (o * np.sum(W * dk) / ell[0]) / (2 * m)]
    go = [sigmoid(raw[L]) * np.sum(W * k) / (2 * m)] if S else []
    grad = np.array(gl + go + [sigmoid(raw[L + S]) * np.trace(w[:, None] * W) / (2 * m), -np.sum(alpha) / m], dtype=dtype)
    return dict(loss=loss, grad=grad, Kinv=Kinv, alpha=alpha, K=K, k=k, dk=dk, t=t, u2=u2, res=res, logdiag=logdiag, ell=ell, o=o, n=n)


def gp2_train_noise(P0, y, kernel, flags, w, v, lr=0.1, max_iter=1000, tol=1e-5, raw0=None, dtype=np.float64, route='chol'):
    """gp2_train over gp2_loss_grad_noise: the loop of one mode, Adam's moments, loss_old and the counters starting afresh at
    raw0.  -> dict(raw (after the last step), iterations, loss, e (of the last evaluation), trace (iterations, 1 + n_par),
    es (e of every evaluation))"""
    T = np.dtype(dtype).type
    n_par = layout(P0.shape[1], flags)[2]
    p = np.zeros(n_par, dtype=dtype) if raw0 is None else np.array(raw0, dtype=dtype)
    m1, m2 = np.zeros(n_par, dtype=dtype), np.zeros(n_par, dtype=dtype)
    b1, b2, b1t, b2t = T(0.9), T(0.999), T(1), T(1)
    loss_old, e, j, trace, loss, es = T(1e10), T(1e10), 0, [], T(np.nan), []
    while e > tol and j < max_iter:
        ev = gp2_loss_grad_noise(P0, y, p, kernel, flags, w, v, dtype, route)
        loss, g = ev['loss'], ev['grad']
        e = abs(loss - loss_old)
        es.append(e)
        loss_old = loss
        trace.append(np.concatenate([[loss], p]))
        b1t, b2t = b1t * b1, b2t * b2
        m1 = b1 * m1 + (1 - b1) * g
        m2 = b2 * m2 + (1 - b2) * g * g
        p = p - (T(lr) / (1 - b1t)) * (m1 / (np.sqrt(m2) / np.sqrt(1 - b2t) + T(1e-8)))
        j += 1
    return dict(raw=p, iterations=j, loss=loss, e=e, trace=np.array(trace, dtype=dtype).reshape(-1, 1 + n_par), es=np.array(es))


def noise_case(m, r, seed, k=None):
    """-> w (m,), V (m, r): the last k = max(1, m // 4) points carry a given variance (0.15 + 0.3 u)^2, the others the learned one"""
    k = max(1, m // 4) if k is None else k
    w, V = np.ones(m), np.zeros((m, r))
    w[m - k:] = 0.0
    V[m - k:] = (0.15 + 0.3 * np.random.default_rng(seed).random((k, r))) ** 2
    return w, V


# ------------------------------------------------------------------------------------------------ the engine double
class GpNoiseNumpyEngine(Gp2NumpyEngine):
    """Gp2NumpyEngine + gp_train_noise with the contract of HipEngine's, computed by the oracle"""

    def gp_train_noise(self, P0, Y, w, V, kernel, flags, raw, lr, max_iter, tol, trace=False):
        self._log('gp_train_noise', kernel, flags, max_iter)
        P0n, Yn, wn, Vn, rawn = P0.numpy(), Y.numpy(), w.numpy(), V.numpy(), raw.numpy().copy()
        m, r = Yn.shape
        n_par = layout(P0n.shape[1], flags)[2]
        assert rawn.shape == (r, n_par) and wn.shape == (m,) and Vn.shape == (m, r)
        Kinv, alpha, info = np.empty((r, m, m)), np.empty((r, m)), np.zeros((r, 4 + n_par))
        tr = np.zeros((r, max_iter, 1 + n_par)) if trace and max_iter > 0 else None
        self.launches = getattr(self, 'launches', 0) + 1
        for q in range(r):
            if max_iter > 0:
                t = gp2_train_noise(P0n, Yn[:, q], kernel, flags, wn, Vn[:, q], lr, max_iter, tol, raw0=rawn[q])
                rawn[q] = t['raw']
                info[q, :3] = t['iterations'], t['loss'], t['e']
                info[q, 4:] = gp2_loss_grad_noise(P0n, Yn[:, q], t['trace'][-1, 1:], kernel, flags, wn, Vn[:, q])['grad']
                if tr is not None:
                    tr[q, :t['iterations']] = t['trace']
            try:
                ev = gp2_loss_grad_noise(P0n, Yn[:, q], rawn[q], kernel, flags, wn, Vn[:, q])
            except np.linalg.LinAlgError:
                info[q, 3] = 1
                continue
            Kinv[q], alpha[q] = ev['Kinv'], ev['alpha']
            if max_iter == 0:
                info[q, 1], info[q, 4:] = ev['loss'], ev['grad']
        f = torch.from_numpy
        return f(rawn), f(Kinv), f(alpha), f(info), None if tr is None else f(tr)


GK = GPKernel('matern52', ard=True, scale=True)
P_NEW = np.array([[1.7, 333.0], [2.9, 310.0], [3.8, 349.0]])
P_STAR = np.array([[2.0, 330.0], [1.7, 333.0], [3.3, 341.0]])


def trained(kernel=None, max_iter=20, eng=None, **kw):
    eng = eng or GpNoiseNumpyEngine()
    g = fitted2(eng)
    g.train(kernel=kernel, max_iter=max_iter, **kw)
    return g, eng


def new_data(g, scale=0.01):
    """measured coefficients at P_NEW: the prediction plus a perturbation, and standard deviations of that size"""
    rng = np.random.default_rng(1)
    amax = np.abs(g.Ar).max()
    return g.predict(P_NEW)[0] + scale * amax * rng.standard_normal((3, 3)), scale * amax * (0.5 + rng.random((3, 3)))


def _close(a, b, rel=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.max(np.abs(a - b)) <= rel * max(np.max(np.abs(b)), 1e-300)


# ------------------------------------------------------------------------------------------------ tests: the oracle
@pytest.mark.parametrize('d', [1, 3])
@pytest.mark.parametrize('flags', [0, 1, 2, 3])
@pytest.mark.parametrize('kernel', KERNELS)
def test_oracle_gradient_against_central_differences(kernel, flags, d):
    m = 12
    P0, Y = gp_case(m, d, 1, seed=5 + d)
    w, V = noise_case(m, 1, seed=d)
    w[2] = 0.5                                                     # the formula holds for any weight
    n_par = layout(d, flags)[2]
    for s in range(3):
        raw = widen(s, d, flags).astype(LD)
        g = gp2_loss_grad_noise(P0, Y[:, 0], raw, kernel, flags, w, V[:, 0], dtype=LD)['grad']
        assert g.shape == (n_par,) and g.dtype == LD
        for c in range(n_par):
            h = np.zeros(n_par, dtype=LD)
            h[c] = LD(1e-5)
            num = (gp2_loss_grad_noise(P0, Y[:, 0], raw + h, kernel, flags, w, V[:, 0], dtype=LD)['loss']
                   - gp2_loss_grad_noise(P0, Y[:, 0], raw - h, kernel, flags, w, V[:, 0], dtype=LD)['loss']) / (2 * h[c])
            assert abs(num - g[c]) <= 1e-7 * max(1, abs(g[c])), (kernel, flags, d, s, c, float(num), float(g[c]))


@pytest.mark.parametrize('dtype', [np.float64, LD])
@pytest.mark.parametrize('flags', [0, 1, 2, 3])
@pytest.mark.parametrize('kernel', KERNELS)
def test_unit_weights_and_no_fixed_noise_are_the_homoscedastic_oracle(kernel, flags, dtype):
    for m, d in ((12, 3), (37, 1), (130, 2)):
        P0, Y = gp_case(m, d, 1, seed=9 + m)
        for s in range(3):
            raw = widen(s, d, flags)
            old = gp2_loss_grad(P0, Y[:, 0], raw, kernel, flags, dtype=dtype)
            new = gp2_loss_grad_noise(P0, Y[:, 0], raw, kernel, flags, np.ones(m), np.zeros(m), dtype=dtype)
            for key in ('loss', 'grad', 'Kinv', 'alpha', 'K', 'logdiag'):
                assert np.array_equal(new[key], old[key]), (key, m, d, s)
    P0, Y = gp_case(15, 2, 1, seed=2)
    a = gp2_train(P0, Y[:, 0], kernel, flags, max_iter=6, tol=0.0, dtype=dtype)
    b = gp2_train_noise(P0, Y[:, 0], kernel, flags, np.ones(15), np.zeros(15), max_iter=6, tol=0.0, dtype=dtype)
    assert np.array_equal(a['trace'], b['trace']) and np.array_equal(a['raw'], b['raw']) and a['e'] == b['e'] == b['es'][-1]


@pytest.mark.parametrize('flags', [0, 3])
def test_the_two_routes_of_the_oracle_agree(flags):
    m, d = 37, 3
    P0, Y = gp_case(m, d, 1, seed=4)
    w, V = noise_case(m, 1, seed=4)
    for s in range(3):
        raw = widen(s, d, flags)
        a = gp2_loss_grad_noise(P0, Y[:, 0], raw, 'matern52', flags, w, V[:, 0])
        b = gp2_loss_grad_noise(P0, Y[:, 0], raw, 'matern52', flags, w, V[:, 0], route='inv')
        assert np.allclose(b['grad'], a['grad'], rtol=1e-9, atol=1e-12) and abs(a['loss'] - b['loss']) < 1e-12
        assert _close(b['Kinv'], a['Kinv'], 1e-10) and b['logdiag'] is None
    # a point with weight 0 has no say in the noise gradient's sum; with no weighted point at all the component is exactly 0
    ev = gp2_loss_grad_noise(P0[:1], Y[:1, 0], widen(0, d, flags), 'matern52', flags, np.zeros(1), np.array([0.04]))
    assert ev['grad'][-2] == 0.0 and ev['K'][0, 0] == float(ev['o']) * 1.0 + 0.04


# ------------------------------------------------------------------------------------------------ tests: update(fixed_noise=True)
def closed_form(g, raw, A_new, A_sigma_new, w=None):
    """K + diag(n) of the plain kernel from the distance matrix, solved: independent of the oracle's factor route.
    -> P0_tot, Kinv (r, m, m), alpha (r, m)"""
    P0_tot = np.concatenate([g.P0, (P_NEW - g.P_cnt[0]) / g.P_scl[0]])
    Y_tot = np.concatenate([g.Vr, A_new / g.Sigma_r])
    m, k = len(g.P0), len(A_new)
    D = gp_distance(P0_tot)
    Kinv, alpha = [], []
    for q in range(g.Vr.shape[1]):
        ell, s2, mu = softplus(raw[q, 0]), softplus(raw[q, 1]) + 1e-4, raw[q, 2]
        n = np.concatenate([np.full(m, s2), (A_sigma_new[:, q] / g.Sigma_r[q]) ** 2])
        K = gp_kernel('matern52', D / ell)[0] + np.diag(n)
        Kinv.append(np.linalg.solve(K, np.eye(m + k)))
        alpha.append(np.linalg.solve(K, Y_tot[:, q] - mu))
    return P0_tot, np.stack(Kinv), np.stack(alpha)


def test_fixed_noise_update_equals_the_closed_form():
    g, eng = trained()
    raw = np.stack([q.raw for q in g.models])
    A_new, A_sig = new_data(g)
    its, e_before = g.gpr_info_['iterations'].copy(), g.gpr_info_['e'].copy()
    g.update(P_NEW, A_new, A_sig, fixed_noise=True)
    assert eng.calls[-1] == ('gp_train_noise', 'matern52', 0, 0)
    assert g.Vr_sigma.shape == (15, 3) and np.all(g.Vr_sigma == 0) and g.gpr_info_['n_train'] == 15 and g.P0.shape == (12, 2)
    assert all(np.array_equal(q.raw, raw[i]) for i, q in enumerate(g.models)) and np.array_equal(g._d['gp_raw'].numpy(), raw)
    assert np.array_equal(g.gpr_info_['iterations'], its) and np.array_equal(g.gpr_info_['e'], e_before)
    assert np.array_equal(g.gpr_info_['noise_weight'], [1.0] * 12 + [0.0] * 3)
    assert g.gpr_info_['fixed_noise'].shape == (15, 3) and np.all(g.gpr_info_['fixed_noise'][:12] == 0)
    assert np.array_equal(g.gpr_info_['fixed_noise'][12:], (A_sig / g.Sigma_r) ** 2)
    P0_tot, Kinv, alpha = closed_form(g, raw, A_new, A_sig)
    assert np.allclose(g._d['gp_Kinv'].numpy(), Kinv, rtol=1e-12, atol=1e-12)
    assert np.allclose(g._d['gp_alpha'].numpy(), alpha, rtol=1e-12, atol=1e-12)
    assert g._d['gp_P0'].shape == (15, 2) and g._d['gp_Y'].shape == (15, 3)
    mean, var = gp_predict(P0_tot, (P_STAR - g.P_cnt[0]) / g.P_scl[0], raw, Kinv, alpha, 'matern52')
    A_pred, A_sigma = g.predict(P_STAR)
    assert np.allclose(A_pred, mean * g.Sigma_r, rtol=1e-12, atol=1e-14) and np.allclose(A_sigma, np.sqrt(var) * g.Sigma_r, rtol=1e-12)
    # loss and gradient describe the new data with its noise at the kept hyper-parameters
    w, V = g.gpr_info_['noise_weight'], g.gpr_info_['fixed_noise']
    Y_tot = np.concatenate([g.Vr, A_new / g.Sigma_r])
    ev = [gp2_loss_grad_noise(P0_tot, Y_tot[:, q], raw[q], 'matern52', 0, w, V[:, q]) for q in range(3)]
    assert np.array_equal(g.gpr_info_['loss'], [e['loss'] for e in ev]) and np.array_equal(g.gpr_info_['grad'], [e['grad'] for e in ev])
    assert [q.loss for q in g.models] == g.gpr_info_['loss'].tolist()
    # device tensors, and a later plain update drops the two keys and takes today's entry point
    Ad, Sd = g.predict(P_STAR, to_host=False)
    assert isinstance(Ad, torch.Tensor) and np.array_equal(Ad.numpy(), A_pred) and np.array_equal(Sd.numpy(), A_sigma)
    g.update(P_NEW, A_new, A_sig)
    assert eng.calls[-1] == ('gp_train', 'matern52', 0) and not {'noise_weight', 'fixed_noise'} & set(g.gpr_info_)


@pytest.mark.parametrize('kernel', [None, GK])
def test_fixed_noise_limits(kernel):
    flags = 0 if kernel is None else kernel.flags
    g, eng = trained(kernel)
    A_new, A_sig = new_data(g, scale=0.05)
    before = g.predict(P_STAR)
    # a measurement with a huge deviation says nothing
    g.update(P_NEW, A_new, np.full((3, 3), 1e6 * np.abs(g.Ar).max()), fixed_noise=True)
    assert eng.calls[-1] == ('gp_train_noise', 'matern52', flags, 0)
    after = g.predict(P_STAR)
    assert _close(after[0], before[0], 1e-9) and _close(after[1], before[1], 1e-9)
    # the learned noise given as a fixed one is the homoscedastic update
    noise = np.array([q.noise for q in g.models])
    g.update(P_NEW, A_new, np.ones((3, 1)) * np.sqrt(noise) * g.Sigma_r, fixed_noise=True)
    fixed = (g._d['gp_Kinv'].numpy(), g._d['gp_alpha'].numpy(), *g.predict(P_STAR))
    g.update(P_NEW, A_new)
    plain = (g._d['gp_Kinv'].numpy(), g._d['gp_alpha'].numpy(), *g.predict(P_STAR))
    assert all(_close(a, b, 1e-12) for a, b in zip(fixed, plain))
    # a smaller deviation of the measurement is a smaller deviation of the prediction there
    g.update(P_NEW, A_new, A_sig, fixed_noise=True)
    wide = g.predict(P_NEW)[1]
    g.update(P_NEW, A_new, 0.1 * A_sig, fixed_noise=True)
    assert np.all(g.predict(P_NEW)[1] < wide)
    g.update(P_NEW[0], A_new[0], np.zeros(3), fixed_noise=True)          # one exact point, given as vectors
    assert g.gpr_info_['n_train'] == 13 and np.all(g.gpr_info_['fixed_noise'][12] == 0)
    A_pred, A_sigma = g.predict(P_NEW[:1])
    assert _close(A_pred, A_new[:1], 1e-10) and _close(A_sigma, np.sqrt(noise) * g.Sigma_r, 1e-6)   # latent variance 0, s2 is added


# ------------------------------------------------------------------------------------------------ tests: update(retrain=True)
@pytest.mark.parametrize('kernel', [None, GK])
def test_retrain_follows_the_warm_started_oracle_loop(kernel, capsys):
    flags = 0 if kernel is None else kernel.flags
    n_par = 3 if kernel is None else kernel.n_par(2)
    g, eng = trained(kernel, max_iter=25, rel_error=1e-4, lr=0.05)
    raw0 = np.stack([q.raw for q in g.models])
    old_models = list(g.models)
    A_new, A_sig = new_data(g, scale=0.05)
    g.update(P_NEW, A_new, A_sig, retrain=True, verbose=True)
    out = capsys.readouterr().out.strip().splitlines()
    assert eng.calls[-1] == ('gp_train_noise', 'matern52', flags, 25)
    P0_tot = np.concatenate([g.P0, (P_NEW - g.P_cnt[0]) / g.P_scl[0]])
    Y_tot = np.concatenate([g.Vr, A_new / g.Sigma_r])
    w, V = np.array([1.0] * 12 + [0.0] * 3), np.concatenate([np.zeros((12, 3)), (A_sig / g.Sigma_r) ** 2])
    assert np.array_equal(g.gpr_info_['noise_weight'], w) and np.array_equal(g.gpr_info_['fixed_noise'], V)
    ts = [gp2_train_noise(P0_tot, Y_tot[:, q], 'matern52', flags, w, V[:, q], lr=0.05, max_iter=25, tol=1e-4, raw0=raw0[q]) for q in range(3)]
    info = g.gpr_info_
    assert info['kernel'] == g.kernel and info['n_train'] == 15 and info['grad'].shape == (3, n_par)
    assert len(out) == sum(t['iterations'] for t in ts)
    t = ts[-1]
    noise = softplus(t['trace'][-1, n_par - 1]) + 1e-4
    assert out[-1] == f'Iter {t["iterations"]}/25 - Mode: 3/3 - Loss: {t["trace"][-1, 0]:.2e} - Mean noise: {noise:.2e}'
    assert g.models is not old_models and g.likelihoods == g.models
    for q, (rec, t) in enumerate(zip(g.models, ts)):
        assert isinstance(rec, GPRecord) and rec is not old_models[q] and rec is g.likelihoods[q]
        assert t['iterations'] >= 2 and not np.array_equal(t['raw'], raw0[q]) and np.array_equal(t['trace'][0, 1:], raw0[q])
        assert np.array_equal(rec.raw, t['raw']) and rec.iterations == t['iterations'] == info['iterations'][q]
        assert rec.loss == t['loss'] == info['loss'][q] and info['e'][q] == t['e'] and rec.status == info['status'][q] == 0
        assert info['converged'][q] == (t['e'] <= 1e-4)
        assert np.array_equal(info['grad'][q], gp2_loss_grad_noise(P0_tot, Y_tot[:, q], t['trace'][-1, 1:], 'matern52', flags, w, V[:, q])['grad'])
        ev = gp2_loss_grad_noise(P0_tot, Y_tot[:, q], t['raw'], 'matern52', flags, w, V[:, q])
        assert np.array_equal(g._d['gp_Kinv'].numpy()[q], ev['Kinv']) and np.array_equal(g._d['gp_alpha'].numpy()[q], ev['alpha'])
    assert np.array_equal(g._d['gp_raw'].numpy(), np.stack([t['raw'] for t in ts]))
    if kernel is None:
        assert np.array_equal(g.Vr_sigma, np.ones((15, 3))) and 'outputscale' not in info
    else:
        assert info['lengthscale'].shape == (3, 2) and np.array_equal(info['outputscale'], [q.outputscale for q in g.models])
        assert np.array_equal(g.Vr_sigma, np.ones((15, 3)) * np.sqrt(info['outputscale']))
    assert g.P0.shape == (12, 2) and g.Vr.shape == (12, 3) and (g.max_iter, g.rel_error, g.lr) == (25, 1e-4, 0.05)
    # predict from the retrained state, the same after a pickle round trip
    want = g.predict(P_STAR)
    assert np.all(np.isfinite(want[0])) and np.all(want[1] > 0)
    if kernel is not None:
        raw = np.stack([t['raw'] for t in ts])
        mean, var = gp2_predict(P0_tot, (P_STAR - g.P_cnt[0]) / g.P_scl[0], raw, g._d['gp_Kinv'].numpy(), g._d['gp_alpha'].numpy(),
                                'matern52', flags)
        assert np.array_equal(want[0], mean * g.Sigma_r) and np.array_equal(want[1], np.sqrt(var) * g.Sigma_r)
    h = pickle.loads(pickle.dumps(g))
    assert set(h._d.stash) >= {'gp_P0', 'gp_Y', 'gp_raw', 'gp_Kinv', 'gp_alpha'}
    h._eng = GpNoiseNumpyEngine()
    got = h.predict(P_STAR)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(h.gpr_info_['noise_weight'], w) and np.array_equal(h.gpr_info_['fixed_noise'], V)
    # quiet without verbose; a second update replaces the data of the first and starts from the retrained values
    g.update(P_NEW[:2], A_new[:2], A_sig[:2], retrain=True)
    assert capsys.readouterr().out == '' and g.gpr_info_['n_train'] == 14 and g.Vr_sigma.shape == (14, 3)


# ------------------------------------------------------------------------------------------------ tests: refusals
def test_refusals_come_before_any_engine_call():
    g, eng = trained(max_iter=3)
    A_new, A_sig = new_data(g)
    state = (g._d['gp_Kinv'], g.gpr_info_['n_train'], g.Vr_sigma.copy(), list(g.models))
    eng.launches = 0
    with pytest.raises(NotImplementedError, match='retrain=True.*A_sigma_new'):
        g.update(P_NEW, A_new, retrain=True)
    with pytest.raises(NotImplementedError, match='retrain=True'):
        g.update(P_NEW, A_new, retrain=True, fixed_noise=True)
    with pytest.raises(ValueError, match='fixed_noise=True.* needs A_sigma_new'):
        g.update(P_NEW, A_new, fixed_noise=True)
    bad = A_sig.copy()
    bad[1, 2] = -1e-3
    nan = A_sig.copy()
    nan[0, 0] = np.nan
    inf = A_sig.copy()
    inf[2, 1] = np.inf
    for kw in (dict(fixed_noise=True), dict(retrain=True)):
        for sig, text in ((bad, 'finite and >= 0'), (nan, 'finite and >= 0'), (inf, 'finite and >= 0'), (A_sig[:2], 'must have shape'),
                          (A_sig[:, :2], 'must have shape'), (A_sig[0], 'must have shape')):
            with pytest.raises(ValueError, match=text):
                g.update(P_NEW, A_new, sig, **kw)
        with pytest.raises(ValueError, match='A_new must have shape'):
            g.update(P_NEW, A_new[:2], A_sig, **kw)
        with pytest.raises(NotImplementedError, match='exceed the 800'):
            g.update(np.ones((800, 2)), np.ones((800, 3)), np.ones((800, 3)), **kw)
    assert eng.launches == 0
    assert g._d['gp_Kinv'] is state[0] and g.gpr_info_['n_train'] == state[1] and np.array_equal(g.Vr_sigma, state[2])
    assert g.models == state[3] and 'noise_weight' not in g.gpr_info_
    fresh = fitted2(GpNoiseNumpyEngine())
    with pytest.raises(AttributeError, match="no attribute 'models'"):
        fresh.update(P_NEW, A_new, A_sig, fixed_noise=True)


@pytest.mark.parametrize('kernel', [None, GK])
def test_engine_without_the_noise_call_is_refused(kernel):
    eng = Gp2NumpyEngine()
    g, _ = trained(kernel, max_iter=2, eng=eng)
    A_new, A_sig = new_data(g)
    n = eng.launches
    for kw in (dict(fixed_noise=True), dict(retrain=True)):
        with pytest.raises(NotImplementedError, match="no 'gp_train_noise' .*no CPU fallback"):
            g.update(P_NEW, A_new, A_sig, **kw)
    assert eng.launches == n
    g.update(P_NEW, A_new, A_sig)                                  # the plain update asks for the plain calls only
    assert g.gpr_info_['n_train'] == 15


def test_contradictory_exact_points_are_not_positive_definite():
    g, _ = trained(max_iter=3)
    A_new, _ = new_data(g)
    with pytest.raises(np.linalg.LinAlgError, match='not positive definite'):
        g.update(np.stack([P_NEW[0], P_NEW[0]]), np.stack([A_new[0], A_new[0] + 1.0]), np.zeros((2, 3)), fixed_noise=True)


# ------------------------------------------------------------------------------------------------ tests: the C entry point
INVALID, UNSUPPORTED = -1, -2
P = [8 * (i + 1) for i in range(10)]
T = 'spr_gp_train_noise_f64'
NAMES = 'P0 m d ldp Y r ldy w V ldv kernel flags raw lr max_iter tol Kinv alpha info trace ws ws_bytes stream'
GOOD = dict(P0=P[0], m=10, d=2, ldp=2, Y=P[1], r=3, ldy=3, w=P[7], V=P[8], ldv=3, kernel=0, flags=3, raw=P[2], lr=0.1, max_iter=5,
            tol=1e-5, Kinv=P[3], alpha=P[4], info=P[5], trace=None, ws=P[6], ws_bytes=1 << 40, stream=None)
D9 = {'d': 9, 'ldp': 9}

CASES = [
    ({'P0': None}, INVALID, 'NULL'), ({'Y': None}, INVALID, 'NULL'), ({'w': None}, INVALID, 'NULL'), ({'V': None}, INVALID, 'NULL'),
    ({'raw': None}, INVALID, 'NULL'), ({'Kinv': None}, INVALID, 'NULL'), ({'alpha': None}, INVALID, 'NULL'),
    ({'info': None}, INVALID, 'NULL'), ({'ws': None}, INVALID, 'NULL'),
    ({'m': 0}, INVALID, 'bad shape'), ({'d': 0}, INVALID, 'bad shape'), ({'r': 0}, INVALID, 'bad shape'),
    ({'ldp': 1}, INVALID, 'bad shape'), ({'ldy': 2}, INVALID, 'bad shape'), ({'max_iter': -1}, INVALID, 'bad shape'),
    ({'ldv': 2}, INVALID, 'bad shape r=3 ldv=2'), ({'ldv': -1}, INVALID, 'bad shape'),
    ({'kernel': 4}, INVALID, 'kernel code'), ({'kernel': -1}, INVALID, 'kernel code'),
    ({'flags': 4}, INVALID, 'flags'), ({'flags': -1}, INVALID, 'flags'),
    ({'lr': 0.0}, INVALID, 'lr'), ({'lr': float('nan')}, INVALID, 'lr'),
    ({'tol': -1.0}, INVALID, 'tol'), ({'tol': float('inf')}, INVALID, 'tol'),
    ({'m': 801}, UNSUPPORTED, 'exceeds 800'),
    (dict(D9, flags=1), UNSUPPORTED, 'd = 9 coordinates exceeds 8'), (dict(D9, flags=3), UNSUPPORTED, 'exceeds 8'),
    (dict(D9, flags=2, ws_bytes='one short'), INVALID, 'workspace of'),      # the scale alone has no cap on d
    (dict(flags=0, ws_bytes='one short'), INVALID, 'workspace of'),           # the plain model takes this entry too
    ({'ws_bytes': 'one short'}, INVALID, 'workspace of'), ({'ws': 12}, INVALID, '8-byte aligned'),
    # order: pointers, shape (ldv last of it), kernel code, flags, step and tolerance, the caps on m and d, the workspace
    ({'w': None, 'm': 0}, INVALID, 'NULL'), ({'V': None, 'ldv': 0}, INVALID, 'NULL'), ({'m': 0, 'ldv': 2}, INVALID, 'bad shape m=0'),
    ({'ldv': 2, 'kernel': 9}, INVALID, 'bad shape r=3 ldv=2'), ({'kernel': 9, 'flags': 7}, INVALID, 'kernel code'),
    ({'flags': 7, 'lr': 0.0}, INVALID, 'flags'), ({'lr': 0.0, 'm': 801}, INVALID, 'lr'),
    (dict(D9, flags=1, m=801), UNSUPPORTED, 'exceeds 800'), ({'m': 801, 'ws_bytes': 0}, UNSUPPORTED, 'exceeds 800'),
    (dict(D9, flags=1, ws_bytes=0), UNSUPPORTED, 'exceeds 8'),
]


@pytest.mark.parametrize('case', CASES, ids=lambda c: '+'.join(f'{k}={v}' for k, v in c[0].items()))
def test_entry_point_refusal(case):
    change, status, fragment = case
    lib = _lib.load()
    args = dict(GOOD, **change)
    if args['ws_bytes'] == 'one short':
        need = lib.spr_gp_workspace_ard(args['m'], args['d'], args['r'])
        assert need == 8 * args['r'] * (2 * args['m'] ** 2 + args['m'] * args['d'])
        args['ws_bytes'] = need - 1
    rc = getattr(lib, T)(*[args[n] for n in NAMES.split()])
    text = lib.spr_last_error().decode()
    assert rc == status, (rc, text)
    assert text.startswith(T + ': ') and fragment in text, text


def test_the_existing_entry_points_refuse_as_before():
    """spr_gp_train_ard_f64 shares its checks with the new entry: it takes no w / V and says nothing of ldv"""
    lib = _lib.load()
    names = 'P0 m d ldp Y r ldy kernel flags raw lr max_iter tol Kinv alpha info trace ws ws_bytes stream'
    args = dict(GOOD, ws_bytes=0)
    rc = lib.spr_gp_train_ard_f64(*[args[n] for n in names.split()])
    text = lib.spr_last_error().decode()
    assert rc == INVALID and text.startswith('spr_gp_train_ard_f64: workspace of 0 bytes'), text
    assert _lib.SPR_ABI_VERSION == 5 and lib.spr_abi_version() == 5
