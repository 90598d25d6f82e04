"""GPR with ARD lengthscales and an output scale on the CPU: the NumPy oracle of the model (gp2_loss_grad, gp2_train,
gp2_predict -- what the ARD kernels of csrc/gp.hip are held to in tests/test_gpr_ard_gpu.py), its gradient against central
differences, its reductions to the oracle of tests/test_gpr_host.py, and the public class over a NumPy double of the two
engine calls.

The model (openmeasure_amd/gpr.py), for flags = ard | scale << 1, L = d if ard else 1, S = 1 if scale else 0, n_par = L + S + 2:
raw = (raw_l[0..L-1], [raw_o], raw_n, mu), l_c = softplus(raw_l[c]) (l_0 for every c when not ard), o = softplus(raw_o) or 1,
s2 = softplus(raw_n) + 1e-4, z_i = P0[i, :] / l, t_ij = max(|z_i - z_j|_2, 1e-15), K = o k(t) + s2 I, alpha = K^-1 (y - mu),
loss = [res.alpha / 2 + log det K / 2 + (m / 2) log 2 pi] / m; with W = K^-1 - alpha alpha^T:
d/d raw_l[c] = sigmoid(raw_l[c]) sum W o dk u_c^2 / t^2 / l_c / 2m (not ard: sum W o dk / l / 2m), d/d raw_o = sigmoid(raw_o) sum W k
/ 2m, d/d raw_n = sigmoid(raw_n) tr W / 2m, d/d mu = -sum alpha / m.  predict: mean = mu + o k*.alpha,
var = max(o - o^2 k*^T K^-1 k*, 0) + s2.

Central differences in longdouble with h = 1e-5: truncation h^2 f''' / 6 ~ 1e-11 times a derivative of order one, rounding
2^-64 |f| / h ~ 1e-14; the gradient check asks for 1e-7 max(1, |g|), the margin for the curvature near the noise floor."""
import pickle

import numpy as np
import pytest
import torch

from openmeasure_amd.gpr import GPR, GPKernel, GPRecord, KERNELS
from tests.test_gpr_host import (GpNumpyEngine, chol_lower, field_case, gp_case, gp_distance, gp_kernel, gp_loss_grad, sigmoid,
                                 softplus, tri_inv_lower)

LD = np.longdouble
LOG_2PI = np.log(2.0 * np.pi)
RAWS = [(0.0, 0.0, 0.0), (-3.0, -9.0, 0.03), (0.8, -3.0, -0.01)]      # (raw_l, raw_n, mu): the start; noise near its floor; long
RAW_O = (0.0, -2.0, 1.5)


# ------------------------------------------------------------------------------------------------ the oracle
def layout(d, flags):
    """-> L, S, n_par"""
    L, S = (d if flags & 1 else 1), (1 if flags & 2 else 0)
    return L, S, L + S + 2


def widen(s, d, flags):
    """setting s of RAWS as n_par values: a distinct raw_l per coordinate (steps of 0.3), raw_o = RAW_O[s]"""
    L, S, _ = layout(d, flags)
    rl, rn, mu = RAWS[s]
    return np.array([rl + 0.3 * c for c in range(L)] + [RAW_O[s]] * S + [rn, mu])


def split(raw, d, flags):
    """-> l (d,), o, s2, mu in raw's dtype"""
    L, S, n_par = layout(d, flags)
    assert len(raw) == n_par
    T = raw.dtype.type
    ell = softplus(raw[:L]) * np.ones(d, dtype=raw.dtype)
    return ell, (softplus(raw[L]) if S else T(1)), softplus(raw[L + S]) + T(1e-4), raw[L + S + 1]


def scaled_t(Za, Zb):
    """t between the rows of Za and Zb, summed coordinate by coordinate, clamped below at 1e-15; -> t, u2 (d, a, b)"""
    u2 = np.stack([(Za[:, c][:, None] - Zb[:, c][None, :]) ** 2 for c in range(Za.shape[1])])
    s = np.zeros(u2.shape[1:], dtype=Za.dtype)
    for c in range(len(u2)):
        s = s + u2[c]
    return np.maximum(np.sqrt(s), Za.dtype.type(1e-15)), u2


def gp2_loss_grad(P0, y, raw, kernel, flags, dtype=np.float64):
    """-> dict(loss, grad (n_par,), Kinv, alpha, K, k, dk, t, u2, res, logdiag, ell, o) at raw"""
    T = np.dtype(dtype).type
    P0, y, raw = np.asarray(P0, dtype=dtype), np.asarray(y, dtype=dtype), np.asarray(raw, dtype=dtype)
    m, d = P0.shape
    L, S, n_par = layout(d, flags)
    ell, o, s2, mu = split(raw, d, flags)
    t, u2 = scaled_t(P0 / ell, P0 / ell)
    k, dk = gp_kernel(kernel, t)
    K = o * k + s2 * np.eye(m, dtype=dtype)
    Lc = np.linalg.cholesky(K) if dtype == np.float64 else chol_lower(K)
    X = tri_inv_lower(Lc)
    Kinv = X.T @ X
    logdiag = 2 * np.log(np.diag(Lc))
    res = y - mu
    alpha = Kinv @ res
    loss = (res @ alpha / 2 + np.sum(logdiag) / 2 + m * T(LOG_2PI) / 2) / m
    W = Kinv - np.outer(alpha, alpha)
    if flags & 1:
        gl = [sigmoid(raw[c]) * (o * np.sum(W * dk * u2[c] / (t * t)) / ell[c]) / (2 * m) for c in range(d)]
    else:
        gl = [sigmoid(raw[0]) * (o * np.sum(W * dk) / ell[0]) / (2 * m)]
    go = [sigmoid(raw[L]) * np.sum(W * k) / (2 * m)] if S else []
    grad = np.array(gl + go + [sigmoid(raw[L + S]) * np.trace(W) / (2 * m), -np.sum(alpha) / m], dtype=dtype)
    return dict(loss=loss, grad=grad, Kinv=Kinv, alpha=alpha, K=K, k=k, dk=dk, t=t, u2=u2, res=res, logdiag=logdiag, ell=ell, o=o)


def gp2_train(P0, y, kernel, flags, lr=0.1, max_iter=1000, tol=1e-5, raw0=None, dtype=np.float64):
    """The training loop of one mode.  -> dict(raw (after the last step), iterations, loss, e (of the last evaluation),
    trace (iterations, 1 + n_par) = (loss, raw) per evaluation)"""
    T = np.dtype(dtype).type
    n_par = layout(P0.shape[1], flags)[2]
    p = np.zeros(n_par, dtype=dtype) if raw0 is None else np.array(raw0, dtype=dtype)
    m1, m2 = np.zeros(n_par, dtype=dtype), np.zeros(n_par, dtype=dtype)
    b1, b2, b1t, b2t = T(0.9), T(0.999), T(1), T(1)
    loss_old, e, j, trace, loss = T(1e10), T(1e10), 0, [], T(np.nan)
    while e > tol and j < max_iter:
        ev = gp2_loss_grad(P0, y, p, kernel, flags, dtype)
        loss, g = ev['loss'], ev['grad']
        e = abs(loss - loss_old)
        loss_old = loss
        trace.append(np.concatenate([[loss], p]))
        b1t, b2t = b1t * b1, b2t * b2
        m1 = b1 * m1 + (1 - b1) * g
        m2 = b2 * m2 + (1 - b2) * g * g
        p = p - (T(lr) / (1 - b1t)) * (m1 / (np.sqrt(m2) / np.sqrt(1 - b2t) + T(1e-8)))
        j += 1
    return dict(raw=p, iterations=j, loss=loss, e=e, trace=np.array(trace, dtype=dtype).reshape(-1, 1 + n_par))


def gp2_predict(P0, Pstar, raw, Kinv, alpha, kernel, flags):
    """raw (r, n_par), Kinv (r, m, m), alpha (r, m) -> mean, var (n_p, r); var includes the noise"""
    Pstar = np.asarray(Pstar, dtype=P0.dtype)
    mean, var = np.empty((len(Pstar), len(raw)), dtype=P0.dtype), np.empty((len(Pstar), len(raw)), dtype=P0.dtype)
    for q in range(len(raw)):
        ell, o, s2, mu = split(raw[q], P0.shape[1], flags)
        ks = gp_kernel(kernel, scaled_t(Pstar / ell, P0 / ell)[0])[0]
        mean[:, q] = mu + o * (ks @ alpha[q])
        var[:, q] = np.maximum(o - o * o * np.einsum('pi,ij,pj->p', ks, Kinv[q], ks), 0) + s2
    return mean, var


# ------------------------------------------------------------------------------------------------ the engine double
class Gp2NumpyEngine(GpNumpyEngine):
    """GpNumpyEngine + the two ARD / scaled calls with the contract of HipEngine's, computed by the oracle.  ``calls`` lists
    every GP call made, with its kernel and iteration count."""

    def _log(self, *what):
        self.__dict__.setdefault('calls', []).append(what)

    def gp_train(self, P0, Y, kernel, raw, lr, max_iter, tol, trace=False):
        self._log('gp_train', kernel, max_iter)
        return super().gp_train(P0, Y, kernel, raw, lr, max_iter, tol, trace=trace)

    def gp_predict(self, P0, Pstar, kernel, raw, Kinv, alpha):
        self._log('gp_predict', kernel, len(Pstar))
        return super().gp_predict(P0, Pstar, kernel, raw, Kinv, alpha)

    def gp_train_ard(self, P0, Y, kernel, flags, raw, lr, max_iter, tol, trace=False):
        self._log('gp_train_ard', kernel, flags, max_iter)
        P0n, Yn, rawn = P0.numpy(), Y.numpy(), raw.numpy().copy()
        m, r = Yn.shape
        n_par = layout(P0n.shape[1], flags)[2]
        assert rawn.shape == (r, n_par)
        Kinv, alpha, info = np.empty((r, m, m)), np.empty((r, m)), np.zeros((r, 4 + n_par))
        tr = np.zeros((r, max_iter, 1 + n_par)) if trace and max_iter > 0 else None
        self.launches = getattr(self, 'launches', 0) + 1
        for q in range(r):
            if max_iter > 0:
                t = gp2_train(P0n, Yn[:, q], kernel, flags, lr, max_iter, tol, raw0=rawn[q])
                rawn[q] = t['raw']
                info[q, :3] = t['iterations'], t['loss'], t['e']
                info[q, 4:] = gp2_loss_grad(P0n, Yn[:, q], t['trace'][-1, 1:], kernel, flags)['grad']
                if tr is not None:
                    tr[q, :t['iterations']] = t['trace']
            try:
                ev = gp2_loss_grad(P0n, Yn[:, q], rawn[q], kernel, flags)
            except np.linalg.LinAlgError:
                info[q, 3] = 1
                continue
            Kinv[q], alpha[q] = ev['Kinv'], ev['alpha']
            if max_iter == 0:
                info[q, 1], info[q, 4:] = ev['loss'], ev['grad']
        f = torch.from_numpy
        return f(rawn), f(Kinv), f(alpha), f(info), None if tr is None else f(tr)

    def gp_predict_ard(self, P0, Pstar, kernel, flags, raw, Kinv, alpha):
        self._log('gp_predict_ard', kernel, flags, len(Pstar))
        self.launches = getattr(self, 'launches', 0) + 1
        mean, var = gp2_predict(P0.numpy(), Pstar.numpy(), raw.numpy(), Kinv.numpy(), alpha.numpy(), kernel, flags)
        return torch.from_numpy(mean), torch.from_numpy(var)


def fitted2(engine=None, r=3, **kw):
    X, F, P = field_case(**kw)
    g = GPR(X, F, None, P, engine=engine or Gp2NumpyEngine())
    g.fit(select_modes='number', n_modes=r)
    return g


# ------------------------------------------------------------------------------------------------ tests: the oracle
@pytest.mark.parametrize('d', [1, 3])
@pytest.mark.parametrize('flags', [1, 2, 3])
@pytest.mark.parametrize('kernel', KERNELS)
def test_oracle_gradient_against_central_differences(kernel, flags, d):
    P0, Y = gp_case(12, d, 1, seed=5 + d)
    n_par = layout(d, flags)[2]
    for s in range(3):
        raw = widen(s, d, flags).astype(LD)
        g = gp2_loss_grad(P0, Y[:, 0], raw, kernel, flags, dtype=LD)['grad']
        assert g.shape == (n_par,) and g.dtype == LD
        for c in range(n_par):
            h = np.zeros(n_par, dtype=LD)
            h[c] = LD(1e-5)
            num = (gp2_loss_grad(P0, Y[:, 0], raw + h, kernel, flags, dtype=LD)['loss']
                   - gp2_loss_grad(P0, Y[:, 0], raw - h, kernel, flags, dtype=LD)['loss']) / (2 * h[c])
            assert abs(num - g[c]) <= 1e-7 * max(1, abs(g[c])), (kernel, flags, d, s, c, float(num), float(g[c]))


def _close(a, b, rel=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.max(np.abs(a - b)) <= rel * max(np.max(np.abs(b)), 1e-300)


@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('d', [1, 3])
def test_oracle_reduces_to_the_plain_oracle(kernel, d):
    P0, Y = gp_case(12, d, 1, seed=9 + d)
    D = gp_distance(P0)
    for rl, rn, mu in RAWS:
        old = gp_loss_grad(D, Y[:, 0], np.array([rl, rn, mu]), kernel)
        # flags = 0: the same model (the gradient relative to its largest component: on the diagonal the plain oracle clamps
        # the distance before the division by l, this one after, a difference of dk(1e-15 / l) - dk(1e-15) per point)
        new = gp2_loss_grad(P0, Y[:, 0], np.array([rl, rn, mu]), kernel, 0)
        assert all(_close(new[k], old[k]) for k in ('loss', 'Kinv', 'alpha')) and _close(new['grad'], old['grad'])
        # scale with raw_o = log(e - 1): o = 1
        one = gp2_loss_grad(P0, Y[:, 0], np.array([rl, np.log(np.e - 1), rn, mu]), kernel, 2)
        assert abs(float(one['o']) - 1) < 1e-15 and all(_close(one[k], old[k]) for k in ('loss', 'Kinv', 'alpha'))
        assert _close(one['grad'][[0, 2, 3]], old['grad'])
        # ard with every raw_l equal: the d lengthscale gradients sum to the isotropic one -- to 1e-12 of the sum of ABSOLUTE
        # terms (the gradient itself cancels to far less near the floor), plus the one term in which the models differ: on the
        # diagonal the plain oracle sees dk at the clamped distance over l, t = 1e-15 / l (dk = t for Matern-1/2), ARD an exact 0
        ard = gp2_loss_grad(P0, Y[:, 0], np.array([rl] * d + [rn, mu]), kernel, 1)
        W = old['Kinv'] - np.outer(old['alpha'], old['alpha'])
        pre = sigmoid(np.float64(rl)) / softplus(np.float64(rl)) / (2 * len(P0))
        bar = 1e-12 * pre * np.sum(np.abs(W * old['dk'])) + pre * np.sum(np.abs(np.diag(W))) * gp_kernel(kernel, 1e-15 / softplus(np.float64(rl)))[1]
        assert _close(ard['loss'], old['loss']) and abs(np.sum(ard['grad'][:d]) - old['grad'][0]) <= bar
        assert _close(ard['grad'][d:], old['grad'][1:])


def test_oracle_training_loop_and_predict():
    P0, Y = gp_case(15, 2, 1, seed=2)
    t = gp2_train(P0, Y[:, 0], 'matern52', 3, max_iter=7, tol=0.0)
    assert t['iterations'] == 7 and t['trace'].shape == (7, 6) and np.all(t['trace'][0, 1:] == 0)
    assert np.allclose(np.abs(t['trace'][1, 1:]), 0.1, rtol=1e-4)          # Adam's first step is lr g / (|g| + 1e-8)
    ev = gp2_loss_grad(P0, Y[:, 0], t['raw'], 'matern52', 3)
    Ps = np.stack([P0[4], P0.mean(axis=0) + 1000.0])
    mean, var = gp2_predict(P0, Ps, t['raw'][None], ev['Kinv'][None], ev['alpha'][None], 'matern52', 3)
    ell, o, s2, mu = split(t['raw'], 2, 3)
    assert abs(var[1, 0] - (o + s2)) <= 1e-15 * (o + s2) and mean[1, 0] == mu       # far away: the prior
    assert s2 <= var[0, 0] < 2 * s2 + 1e-3                                          # at a training point: about the noise


# ------------------------------------------------------------------------------------------------ tests: the class
def test_gpkernel_is_a_small_value():
    k = GPKernel('rbf', ard=True)
    assert (k.name, k.ard, k.scale, k.flags) == ('rbf', True, False, 1) and GPKernel().name == 'matern52' and GPKernel().flags == 0
    assert GPKernel('matern32', scale=True).flags == 2 and GPKernel('matern12', True, True).flags == 3
    assert k == GPKernel('rbf', True, False) and k != GPKernel('rbf') and k != 'rbf' and hash(k) == hash(GPKernel('rbf', 1, 0))
    assert len({k, GPKernel('rbf', True), GPKernel('rbf', scale=True)}) == 2
    assert repr(k) == "GPKernel('rbf', ard=True, scale=False)" and eval(repr(k)) == k
    assert pickle.loads(pickle.dumps(k)) == k
    with pytest.raises(AttributeError):
        k.ard = False
    for bad in ('matern', 'periodic', None, 5):
        with pytest.raises(ValueError, match='must be one of'):
            GPKernel(bad)
    assert k.n_par(3) == 5 and GPKernel('rbf', scale=True).n_par(3) == 4 and GPKernel('rbf', True, True).n_par(3) == 6


@pytest.mark.parametrize('flags', [1, 2, 3])
def test_train_predict_update_pickle(flags):
    eng = Gp2NumpyEngine()
    g = fitted2(eng)
    gk = GPKernel('matern32', ard=bool(flags & 1), scale=bool(flags & 2))
    L, S, n_par = layout(2, flags)
    models, likelihoods = g.train(kernel=gk, max_iter=40)
    assert g.kernel is gk and g.gpr_info_['kernel'] is gk and g.models is models and g.likelihoods is likelihoods
    assert [c[0] for c in eng.calls] == ['gp_train_ard'] and eng.calls[0][1:] == ('matern32', flags, 40)
    info = g.gpr_info_
    assert info['grad'].shape == (3, n_par) and info['lengthscale'].shape == (3, L) and info['outputscale'].shape == (3,)
    assert info['iterations'].shape == info['loss'].shape == info['e'].shape == info['status'].shape == info['converged'].shape == (3,)
    assert info['n_train'] == 12
    for i, rec in enumerate(models):
        t = gp2_train(g.P0, g.Vr[:, i], 'matern32', flags, max_iter=40)
        assert isinstance(rec, GPRecord) and rec.raw.shape == (n_par,) and np.array_equal(rec.raw, t['raw'])
        assert rec.iterations == t['iterations'] == info['iterations'][i] and rec.loss == t['loss'] and rec.status == 0
        if flags & 1:
            assert isinstance(rec.lengthscale, np.ndarray) and rec.lengthscale.shape == (2,)
            assert np.allclose(rec.lengthscale, softplus(t['raw'][:2]), rtol=4e-16, atol=0)
        else:
            assert isinstance(rec.lengthscale, float) and rec.lengthscale == pytest.approx(softplus(t['raw'][0]), rel=4e-16)
        assert isinstance(rec.outputscale, float) and rec.outputscale == (pytest.approx(softplus(t['raw'][L]), rel=4e-16) if S else 1.0)
        assert rec.noise == pytest.approx(softplus(t['raw'][L + S]) + 1e-4, rel=4e-16) and rec.mean == t['raw'][L + S + 1]
        assert isinstance(rec.noise, float) and isinstance(rec.mean, float) and 'outputscale' in repr(rec)
        assert np.array_equal(info['lengthscale'][i], np.atleast_1d(rec.lengthscale)) and info['outputscale'][i] == rec.outputscale
        assert np.array_equal(info['grad'][i], gp2_loss_grad(g.P0, g.Vr[:, i], t['trace'][-1, 1:], 'matern32', flags)['grad'])
    assert g.Vr_sigma.shape == (12, 3) and np.array_equal(g.Vr_sigma, np.ones((12, 3)) * np.sqrt(info['outputscale']))
    # predict = the oracle's closed form times Sigma_r
    raw = np.stack([q.raw for q in models])
    ev = [gp2_loss_grad(g.P0, g.Vr[:, i], raw[i], 'matern32', flags) for i in range(3)]
    P_star = np.array([[2.2, 320.0], [3.3, 341.0]])
    P0s = (P_star - g.P_cnt[0]) / g.P_scl[0]
    mean, var = gp2_predict(g.P0, P0s, raw, np.stack([e['Kinv'] for e in ev]), np.stack([e['alpha'] for e in ev]), 'matern32', flags)
    A_pred, A_sigma = g.predict(P_star)
    assert np.array_equal(A_pred, mean * g.Sigma_r) and np.array_equal(A_sigma, np.sqrt(var) * g.Sigma_r)
    assert eng.calls[-1] == ('gp_predict_ard', 'matern32', flags, 2)
    X_rec, X_std = g.reconstruct(A_pred), g.reconstruct_std(A_sigma)
    assert X_rec.shape == X_std.shape == (201, 2) and np.all(np.isfinite(X_rec)) and np.all(X_std > 0)
    Ad, Sd = g.predict(P_star, to_host=False)
    assert isinstance(Ad, torch.Tensor) and np.array_equal(Ad.numpy(), A_pred) and np.array_equal(Sd.numpy(), A_sigma)
    assert np.array_equal(g.reconstruct_std(Sd), X_std) and np.array_equal(g.reconstruct(Ad), X_rec)
    # pickle round trip: the same prediction from the restored state
    h = pickle.loads(pickle.dumps(g))
    assert set(h._d.stash) >= {'gp_P0', 'gp_Y', 'gp_raw', 'gp_Kinv', 'gp_alpha'} and h.kernel == gk
    h._eng = Gp2NumpyEngine()
    got = h.predict(P_star)
    assert np.array_equal(got[0], A_pred) and np.array_equal(got[1], A_sigma)
    assert [q.raw.tolist() for q in h.models] == [q.raw.tolist() for q in models]
    assert all(np.array_equal(a.lengthscale, b.lengthscale) and a.outputscale == b.outputscale for a, b in zip(h.models, models))
    # update: one factorisation of the concatenated data at the kept hyper-parameters
    P_new = np.array([[1.7, 333.0], [2.9, 310.0], [3.8, 349.0]])
    A_new = g.predict(P_new)[0] + 0.01 * np.abs(g.Ar).max() * np.random.default_rng(1).standard_normal((3, 3))
    before, its = g.predict(P_new)[1], info['iterations'].copy()
    g.update(P_new, A_new, A_sigma_new=np.ones((3, 3)))
    assert eng.calls[-1] == ('gp_train_ard', 'matern32', flags, 0)
    assert g.Vr_sigma.shape == (15, 3) and np.all(g.Vr_sigma == 0) and g.gpr_info_['n_train'] == 15 and g.P0.shape == (12, 2)
    assert all(np.array_equal(q.raw, raw[i]) for i, q in enumerate(g.models)) and np.array_equal(g.gpr_info_['iterations'], its)
    P0_tot = np.concatenate([g.P0, (P_new - g.P_cnt[0]) / g.P_scl[0]])
    Y_tot = np.concatenate([g.Vr, A_new / g.Sigma_r])
    ev = [gp2_loss_grad(P0_tot, Y_tot[:, i], raw[i], 'matern32', flags) for i in range(3)]
    assert np.array_equal(g._d['gp_Kinv'].numpy(), np.stack([e['Kinv'] for e in ev]))
    assert np.array_equal(g.gpr_info_['loss'], [e['loss'] for e in ev]) and g.gpr_info_['grad'].shape == (3, n_par)
    assert np.array_equal(g.gpr_info_['grad'], np.stack([e['grad'] for e in ev]))
    assert [q.loss for q in g.models] == g.gpr_info_['loss'].tolist()
    mean, var = gp2_predict(P0_tot, P0s, raw, np.stack([e['Kinv'] for e in ev]), np.stack([e['alpha'] for e in ev]), 'matern32', flags)
    A_pred, A_sigma = g.predict(P_star)
    assert np.array_equal(A_pred, mean * g.Sigma_r) and np.array_equal(A_sigma, np.sqrt(var) * g.Sigma_r)
    assert np.all(g.predict(P_new)[1] < before)                # data at a point lowers the uncertainty there


def test_verbose_prints_the_reference_line_from_the_wider_trace(capsys):
    g = fitted2(r=2)
    g.train(kernel=GPKernel('matern52', ard=True, scale=True), max_iter=3, rel_error=0.0, verbose=True)
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 6
    t = gp2_train(g.P0, g.Vr[:, 1], 'matern52', 3, max_iter=3, tol=0.0)
    noise = softplus(t['trace'][2, 4]) + 1e-4
    assert out[-1] == f'Iter 3/3 - Mode: 2/2 - Loss: {t["trace"][2, 0]:.2e} - Mean noise: {noise:.2e}'


def test_unflagged_gpkernel_takes_the_existing_path():
    ea, eb = Gp2NumpyEngine(), Gp2NumpyEngine()
    a, b = fitted2(ea), fitted2(eb)
    a.train(kernel='rbf', max_iter=20)
    b.train(kernel=GPKernel('rbf'), max_iter=20)
    P_star = np.array([[2.2, 320.0], [3.3, 341.0]])
    pa, pb = a.predict(P_star), b.predict(P_star)
    a.update(P_star, pa[0])
    b.update(P_star, pb[0])
    assert ea.calls == eb.calls == [('gp_train', 'rbf', 20), ('gp_predict', 'rbf', 2), ('gp_train', 'rbf', 0)]
    assert np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1])
    assert all(np.array_equal(x.raw, y.raw) and type(y.lengthscale) is float and x.loss == y.loss for x, y in zip(a.models, b.models))
    assert a.kernel == 'rbf' and b.kernel == GPKernel('rbf') and np.array_equal(a.Vr_sigma, b.Vr_sigma)
    assert set(a.gpr_info_) == set(b.gpr_info_) and b.gpr_info_['grad'].shape == (3, 3)
    assert np.array_equal(a._d['gp_Kinv'].numpy(), b._d['gp_Kinv'].numpy())


def test_refusals_come_before_any_engine_call():
    rng = np.random.default_rng(0)
    X, F, _ = field_case()
    eng = Gp2NumpyEngine()
    g = GPR(X, F, None, 1.0 + rng.random((12, 9)), engine=eng)
    g.fit(select_modes='number', n_modes=2)
    eng.launches = 0
    with pytest.raises(NotImplementedError, match='ARD over 9 parameters exceeds the 8'):
        g.train(kernel=GPKernel('matern52', ard=True, scale=True))
    assert eng.launches == 0 and not hasattr(g, 'models') and not getattr(eng, 'calls', [])
    g.train(kernel=GPKernel('matern52', scale=True), max_iter=2)           # the scale alone has no limit on d
    assert g.models[0].raw.shape == (4,)
    with pytest.raises(ValueError, match='must be one of'):
        g.train(kernel=GPKernel('matern'))
    h = fitted2(eng)
    eng.launches = 0
    for kw in (dict(kernel='matern'), dict(kernel='periodic'), dict(kernel=object()), dict(mean='constant'),
               dict(likelihood=object(), kernel=GPKernel('rbf', True))):
        with pytest.raises(NotImplementedError):
            h.train(**kw)
    mt = GPR(X, F, None, field_case()[2], gpr_type='MultiTask', engine=eng)
    mt.fit(select_modes='number', n_modes=2)
    with pytest.raises(NotImplementedError, match='MultiTask'):
        mt.train(kernel=GPKernel('rbf', True))
    assert eng.launches == 0
    h.train(kernel=GPKernel('rbf', True, True), max_iter=2)
    with pytest.raises(NotImplementedError, match='retrain=True'):
        h.update(field_case()[2][:1], h.Ar[:1], retrain=True)
    with pytest.raises(NotImplementedError, match='problem_dict'):
        h.predict(field_case()[2], problem_dict={})


def test_engine_without_the_ard_calls_is_refused():
    g = fitted2(GpNumpyEngine())
    g.train(max_iter=2)                                                    # the plain path asks for the plain calls only
    with pytest.raises(NotImplementedError, match="no 'gp_train_ard' .*no CPU fallback"):
        g.train(kernel=GPKernel('matern52', ard=True))


def test_record_from_three_raws_is_unchanged():
    rec = GPRecord([0.3, -1.0, 0.02], 7, 1.5, 0)
    assert type(rec.lengthscale) is float and rec.lengthscale == float(softplus(np.float64(0.3))) and rec.outputscale == 1.0
    assert rec.noise == float(softplus(np.float64(-1.0)) + 1e-4) and rec.mean == 0.02 and rec.iterations == 7 and rec.status == 0
    assert repr(rec).startswith('GPRecord(lengthscale=') and 'outputscale' not in repr(rec)
    with pytest.raises(ValueError):
        GPRecord([0.0] * 5, 0, 0.0, 0)


# ------------------------------------------------------------------------------------------------ what the feature is for
def relevance_case(m=40, r=3, seed=1):
    """gp_case-style targets that depend on the FIRST of d = 2 scaled parameters only"""
    rng = np.random.default_rng(seed)
    P0 = rng.standard_normal((m, 2))
    Y = np.empty((m, r))
    for q in range(r):
        w = rng.standard_normal()
        Y[:, q] = np.sin((q % 3 + 1) * 0.7 * w * P0[:, 0] + q) + 0.3 * rng.standard_normal() * P0[:, 0] + 0.05 * rng.standard_normal(m)
    return P0, Y / np.linalg.norm(Y, axis=0)


def test_ard_finds_the_irrelevant_parameter_and_the_scale_finds_the_amplitude():
    """Targets that vary with P0[:, 0] only, unit-norm columns (entries of size 1 / sqrt(40)): the ARD + scale kernel ends with
    a longer lengthscale along the parameter that does nothing, a lower loss than the plain kernel, and an output scale below
    the fixed prior variance 1, in every mode."""
    P0, Y = relevance_case()
    for q in range(Y.shape[1]):
        full = gp2_train(P0, Y[:, q], 'matern52', 3)
        plain = gp2_train(P0, Y[:, q], 'matern52', 0)
        rec = GPRecord(full['raw'], full['iterations'], full['loss'], 0, ard=True, scale=True)
        print(f'mode {q}: lengthscale {rec.lengthscale.tolist()}, outputscale {rec.outputscale:.4f}, loss {rec.loss:.4f} after '
              f'{rec.iterations} evaluations; plain kernel: lengthscale {float(softplus(plain["raw"][0])):.4f}, loss '
              f'{float(plain["loss"]):.4f} after {plain["iterations"]}')
        assert rec.lengthscale[1] > rec.lengthscale[0]
        assert rec.loss < plain['loss']
        assert rec.outputscale < 1
