"""GPR on the CPU: the NumPy oracle of the exact-GP model (gp_loss_grad, gp_train, gp_predict -- what csrc/gp.hip is held
to in tests/test_gpr_gpu.py), its gradient against central differences, and the public class over a NumPy double of the
two engine calls.

The model (openmeasure_amd/gpr.py): raw = (raw_l, raw_n, mu), l = softplus(raw_l), s2 = softplus(raw_n) + 1e-4,
K = k(D / l) + s2 I, alpha = K^-1 (y - mu), loss = [res.alpha / 2 + log det K / 2 + (m / 2) log 2 pi] / m; with
W = K^-1 - alpha alpha^T: d/d raw_l = sigmoid(raw_l) sum W o dK/dl / 2m, d/d raw_n = sigmoid(raw_n) tr W / 2m, d/d mu =
-sum alpha / m.  Adam with beta = (0.9, 0.999), eps = 1e-8, bias correction, and the reference's loop (gpr.py:230-247).

Central differences with h = 1e-5 on a loss of order 1: truncation h^2 |f'''| / 6 ~ 1e-10, rounding eps |f| / h ~ 1e-11;
the gradient check asks for 1e-8 (1 + |g|)."""
import pickle

import numpy as np
import pytest
import torch

from openmeasure_amd.gpr import GPR, GPRecord, KERNELS
from tests.test_field_std_host import FieldStdNumpyEngine

LOG_2PI = np.log(2.0 * np.pi)


# ------------------------------------------------------------------------------------------------ the oracle
def softplus(x):
    return np.where(x > 0, x + np.log1p(np.exp(-np.abs(x))), np.log1p(np.exp(-np.abs(x))))[()]


def sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1 / (1 + e), e / (1 + e))[()]


def gp_distance(P, Q=None):
    """Euclidean distances of the rows of P (to those of Q), summed coordinate by coordinate, clamped below at 1e-15"""
    Q = P if Q is None else Q
    s = np.zeros((P.shape[0], Q.shape[0]), dtype=P.dtype)
    for c in range(P.shape[1]):
        v = P[:, c][:, None] - Q[:, c][None, :]
        s = s + v * v
    return np.maximum(np.sqrt(s), P.dtype.type(1e-15))


def gp_kernel(kernel, t):
    """k(t) and l dK/dl at t = D / l, in t's dtype"""
    T = t.dtype.type
    if kernel == 'matern52':
        s = np.sqrt(T(5)) * t
        e = np.exp(-s)
        return (1 + s + (T(5) / T(3)) * t * t) * e, (T(5) / T(3)) * t * t * (1 + s) * e
    if kernel == 'matern32':
        s = np.sqrt(T(3)) * t
        e = np.exp(-s)
        return (1 + s) * e, s * s * e
    if kernel == 'matern12':
        e = np.exp(-t)
        return e, t * e
    assert kernel == 'rbf'
    e = np.exp(-t * t / 2)
    return e, t * t * e


def chol_lower(K):
    """K = L L^T in K's dtype (longdouble has no LAPACK)"""
    m = len(K)
    L = np.zeros_like(K)
    for j in range(m):
        L[j, j] = np.sqrt(K[j, j] - L[j, :j] @ L[j, :j])
        L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def tri_inv_lower(L):
    m = len(L)
    X = np.zeros_like(L)
    for i in range(m):
        X[i, i] = 1 / L[i, i]
        X[i, :i] = -(L[i, :i] @ X[:i, :i]) / L[i, i]
    return X


def gp_loss_grad(D, y, raw, kernel, dtype=np.float64, route='chol'):
    """-> dict(loss, grad (3,), Kinv, alpha, K, dk) at raw = (raw_l, raw_n, mu).  route 'chol': Cholesky factor, its inverse
    X, K^-1 = X^T X; 'inv': numpy.linalg.inv and slogdet (LU; float64 only) -- a different route to the same numbers."""
    T = np.dtype(dtype).type
    D, y, raw = np.asarray(D, dtype=dtype), np.asarray(y, dtype=dtype), np.asarray(raw, dtype=dtype)
    m = len(y)
    ell, s2 = softplus(raw[0]), softplus(raw[1]) + T(1e-4)
    k, dk = gp_kernel(kernel, D / ell)
    K = k + s2 * np.eye(m, dtype=dtype)
    if route == 'chol':
        L = np.linalg.cholesky(K) if dtype == np.float64 else chol_lower(K)
        X = tri_inv_lower(L)
        Kinv = X.T @ X
        logdet = 2 * np.sum(np.log(np.diag(L)))
    else:
        Kinv = np.linalg.inv(K)
        logdet = np.linalg.slogdet(K)[1]
    res = y - raw[2]
    alpha = Kinv @ res
    loss = (res @ alpha / 2 + logdet / 2 + m * T(LOG_2PI) / 2) / m
    W = Kinv - np.outer(alpha, alpha)
    grad = np.array([sigmoid(raw[0]) * (np.sum(W * dk) / ell) / (2 * m), sigmoid(raw[1]) * np.trace(W) / (2 * m),
                     -np.sum(alpha) / m], dtype=dtype)
    return dict(loss=loss, grad=grad, Kinv=Kinv, alpha=alpha, K=K, dk=dk, res=res, logdiag=2 * np.log(np.diag(L)) if route == 'chol'
                else None)


def gp_train(D, y, kernel, lr=0.1, max_iter=1000, tol=1e-5, raw0=(0.0, 0.0, 0.0), dtype=np.float64, route='chol'):
    """The training loop of one mode.  -> dict(raw (after the last step), iterations, loss, e (of the last evaluation),
    trace (iterations, 4) = (loss, raw) per evaluation)"""
    T = np.dtype(dtype).type
    p = np.array(raw0, dtype=dtype)
    m1, m2 = np.zeros(3, dtype=dtype), np.zeros(3, dtype=dtype)
    b1, b2, b1t, b2t = T(0.9), T(0.999), T(1), T(1)
    loss_old, e, j, trace, loss = T(1e10), T(1e10), 0, [], T(np.nan)
    while e > tol and j < max_iter:
        ev = gp_loss_grad(D, y, p, kernel, dtype, route)
        loss, g = ev['loss'], ev['grad']
        e = abs(loss - loss_old)
        loss_old = loss
        trace.append(np.concatenate([[loss], p]))
        b1t, b2t = b1t * b1, b2t * b2
        m1 = b1 * m1 + (1 - b1) * g
        m2 = b2 * m2 + (1 - b2) * g * g
        p = p - (T(lr) / (1 - b1t)) * (m1 / (np.sqrt(m2) / np.sqrt(1 - b2t) + T(1e-8)))
        j += 1
    return dict(raw=p, iterations=j, loss=loss, e=e, trace=np.array(trace, dtype=dtype).reshape(-1, 4))


def gp_predict(P0, Pstar, raw, Kinv, alpha, kernel):
    """raw (r, 3), Kinv (r, m, m), alpha (r, m) -> mean, var (n_p, r); var includes the noise, k(0) = 1"""
    Ds = gp_distance(np.asarray(Pstar, dtype=P0.dtype), P0)
    mean, var = np.empty((len(Ds), len(raw)), dtype=P0.dtype), np.empty((len(Ds), len(raw)), dtype=P0.dtype)
    for q in range(len(raw)):
        ks = gp_kernel(kernel, Ds / softplus(raw[q, 0]))[0]
        mean[:, q] = raw[q, 2] + ks @ alpha[q]
        var[:, q] = np.maximum(1 - np.einsum('pi,ij,pj->p', ks, Kinv[q], ks), 0) + softplus(raw[q, 1]) + P0.dtype.type(1e-4)
    return mean, var


def gp_case(m, d, r, seed=0, noise=0.05):
    """scaled parameters P0 (m, d) and smooth unit-norm targets Y (m, r) with a little noise"""
    rng = np.random.default_rng(seed)
    P0 = rng.standard_normal((m, d))
    Y = np.empty((m, r))
    for q in range(r):
        w = rng.standard_normal(d)
        Y[:, q] = np.sin((q % 3 + 1) * 0.7 * (P0 @ w) + q) + 0.3 * (P0 @ rng.standard_normal(d)) + noise * rng.standard_normal(m)
    return P0, Y / np.maximum(np.linalg.norm(Y, axis=0), 1e-300)


# ------------------------------------------------------------------------------------------------ the engine double
class GpNumpyEngine(FieldStdNumpyEngine):
    """NumpyEngine + the two GP calls with the contract of HipEngine's, computed by the oracle"""

    GP_KERNELS = {k: i for i, k in enumerate(KERNELS)}

    def gp_train(self, P0, Y, kernel, raw, lr, max_iter, tol, trace=False):
        P0n, Yn, rawn = P0.numpy(), Y.numpy(), raw.numpy().copy()
        m, r = Yn.shape
        D = gp_distance(P0n)
        Kinv, alpha, info = np.empty((r, m, m)), np.empty((r, m)), np.zeros((r, 8))
        tr = np.zeros((r, max_iter, 4)) if trace and max_iter > 0 else None
        self.launches = getattr(self, 'launches', 0) + 1
        for q in range(r):
            if max_iter > 0:
                t = gp_train(D, Yn[:, q], kernel, lr, max_iter, tol, raw0=rawn[q])
                rawn[q] = t['raw']
                info[q, :3] = t['iterations'], t['loss'], t['e']
                if tr is not None:
                    tr[q, :t['iterations']] = t['trace']
            try:
                ev = gp_loss_grad(D, Yn[:, q], rawn[q], kernel)
            except np.linalg.LinAlgError:
                info[q, 3] = 1
                continue
            Kinv[q], alpha[q] = ev['Kinv'], ev['alpha']
            if max_iter == 0:
                info[q, 1], info[q, 4:7] = ev['loss'], ev['grad']
        f = torch.from_numpy
        return f(rawn), f(Kinv), f(alpha), f(info), None if tr is None else f(tr)

    def gp_predict(self, P0, Pstar, kernel, raw, Kinv, alpha):
        self.launches = getattr(self, 'launches', 0) + 1
        mean, var = gp_predict(P0.numpy(), Pstar.numpy(), raw.numpy(), Kinv.numpy(), alpha.numpy(), kernel)
        return torch.from_numpy(mean), torch.from_numpy(var)


def field_case(m=12, d=2, seed=3):
    """201 rows (67 points x 3 features) that vary smoothly with the parameters P (m, d)"""
    rng = np.random.default_rng(seed)
    n_points, F = 67, 3
    P = np.column_stack([np.linspace(1.0, 4.0, m), 300 + 50 * rng.random(m)])[:, :d]
    s = np.linspace(0, 1, n_points)
    X = np.empty((n_points * F, m))
    for f in range(F):
        X[f * n_points:(f + 1) * n_points] = (f + 1) * (np.sin(np.outer(s, P[:, 0]) + f) + 0.01 * np.outer(s * s, P[:, -1])) + 10 * f
    return X + 1e-3 * rng.standard_normal(X.shape), F, P


def fitted(engine=None, r=3, **kw):
    X, F, P = field_case(**kw)
    g = GPR(X, F, None, P, engine=engine or GpNumpyEngine())
    g.fit(select_modes='number', n_modes=r)
    return g


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize('kernel', KERNELS)
def test_oracle_gradient_against_central_differences(kernel):
    P0, Y = gp_case(23, 2, 1, seed=5)
    D = gp_distance(P0)
    for raw in ([0.0, 0.0, 0.0], [-0.7, -2.0, 0.05], [0.9, -6.0, -0.02]):
        raw = np.array(raw)
        g = gp_loss_grad(D, Y[:, 0], raw, kernel)['grad']
        for c in range(3):
            h = np.zeros(3)
            h[c] = 1e-5
            num = (gp_loss_grad(D, Y[:, 0], raw + h, kernel)['loss'] - gp_loss_grad(D, Y[:, 0], raw - h, kernel)['loss']) / 2e-5
            assert abs(num - g[c]) <= 1e-8 * (1 + abs(g[c])), (kernel, raw, c, num, g[c])
        alt = gp_loss_grad(D, Y[:, 0], raw, kernel, route='inv')
        assert np.allclose(alt['grad'], g, rtol=1e-9, atol=1e-12) and abs(alt['loss'] - gp_loss_grad(D, Y[:, 0], raw, kernel)['loss']) < 1e-12


def test_oracle_training_loop_follows_the_reference_loop():
    P0, Y = gp_case(15, 1, 1, seed=2)
    D = gp_distance(P0)
    t = gp_train(D, Y[:, 0], 'matern52', max_iter=7, tol=0.0)
    assert t['iterations'] == 7 and t['trace'].shape == (7, 4) and np.all(t['trace'][0, 1:] == 0)
    assert np.allclose(np.abs(t['trace'][1, 1:]), 0.1, rtol=1e-4)          # Adam's first step is lr g / (|g| + 1e-8)
    t = gp_train(D, Y[:, 0], 'matern52', max_iter=1000, tol=1e-5)
    assert 1 < t['iterations'] < 1000 and t['e'] <= 1e-5
    assert t['trace'][-1, 0] < t['trace'][0, 0]
    assert gp_train(D, Y[:, 0], 'rbf', max_iter=0)['iterations'] == 0


def test_fit_train_predict_reconstruct():
    eng = GpNumpyEngine()
    g = fitted(eng)
    assert g.d == 2 and g.r == 3 and g.P0.shape == (12, 2) and g.scaleX_type == 'std' and g.scaleP_type == 'std'
    models, likelihoods = g.train(max_iter=300)
    assert len(models) == len(likelihoods) == 3 and all(isinstance(q, GPRecord) for q in models)
    assert g.models is models and g.likelihoods is likelihoods
    assert g.Vr_sigma.shape == (12, 3) and np.all(g.Vr_sigma == 1)
    D = gp_distance(g.P0)
    for i, rec in enumerate(models):
        t = gp_train(D, g.Vr[:, i], 'matern52', max_iter=300)
        assert rec.iterations == t['iterations'] == g.gpr_info_['iterations'][i] and np.array_equal(rec.raw, t['raw'])
        assert rec.lengthscale == softplus(t['raw'][0]) and rec.noise == softplus(t['raw'][1]) + 1e-4 and rec.mean == t['raw'][2]
        assert rec.status == 0 and rec.loss == t['loss']
    # at the training parameters the posterior mean returns the coefficients to within the noise level
    A_pred, A_sigma = g.predict(g.P)
    assert A_pred.shape == A_sigma.shape == (12, 3)
    assert np.max(np.abs(A_pred - g.Ar)) < 0.2 * np.max(np.abs(g.Ar))
    assert np.all(A_sigma > 0)
    raw = np.stack([q.raw for q in models])
    ev = [gp_loss_grad(D, g.Vr[:, i], raw[i], 'matern52') for i in range(3)]
    mean, var = gp_predict(g.P0, g.P0, raw, np.stack([e['Kinv'] for e in ev]), np.stack([e['alpha'] for e in ev]), 'matern52')
    assert np.array_equal(A_pred, mean * g.Sigma_r) and np.array_equal(A_sigma, np.sqrt(var) * g.Sigma_r)
    P_star = np.array([[2.2, 320.0], [3.3, 341.0]])
    A_pred, A_sigma = g.predict(P_star)
    X_rec, X_std = g.reconstruct(A_pred), g.reconstruct_std(A_sigma)
    assert X_rec.shape == X_std.shape == (201, 2)
    assert np.allclose(X_rec, g.X_cnt + g.X_scl * (g.Ur @ A_pred.T), rtol=1e-12, atol=1e-12)
    assert np.allclose(X_std, g.X_scl * np.sqrt((g.Ur ** 2) @ (A_sigma ** 2).T), rtol=1e-12, atol=1e-14)
    # device tensors go through the same chain
    Ad, Sd = g.predict(P_star, to_host=False)
    assert isinstance(Ad, torch.Tensor) and np.array_equal(Ad.numpy(), A_pred) and np.array_equal(Sd.numpy(), A_sigma)
    assert np.array_equal(g.reconstruct_std(Sd), X_std)
    # one point given as a vector is one row
    a1, s1 = g.predict(P_star[1])
    # (the double's BLAS products sum in an order that depends on the batch: a few ulp, not bit for bit)
    assert a1.shape == (1, 3) and np.allclose(a1[0], A_pred[1], rtol=1e-13, atol=0) and np.allclose(s1[0], A_sigma[1], rtol=1e-13, atol=0)


@pytest.mark.parametrize('kernel', KERNELS)
def test_every_kernel_trains(kernel):
    g = fitted(r=2)
    g.train(kernel=kernel, max_iter=40)
    assert g.kernel == kernel and g.gpr_info_['kernel'] == kernel
    assert np.all(g.gpr_info_['loss'] < gp_loss_grad(gp_distance(g.P0), g.Vr[:, 0], np.zeros(3), kernel)['loss'] + 1)
    assert np.all(np.isfinite(g.predict(g.P)[0]))


def test_verbose_prints_the_reference_line(capsys):
    g = fitted(r=2)
    g.train(max_iter=3, rel_error=0.0, verbose=True)
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 6
    t = gp_train(gp_distance(g.P0), g.Vr[:, 1], 'matern52', max_iter=3, tol=0.0)
    noise = softplus(t['trace'][2, 2]) + 1e-4
    assert out[-1] == f'Iter 3/3 - Mode: 2/2 - Loss: {t["trace"][2, 0]:.2e} - Mean noise: {noise:.2e}'


SCALINGS = {
    'std': lambda x: np.std(x), 'none': lambda x: 1.0, 'pareto': lambda x: np.sqrt(np.std(x)),
    'vast': lambda x: np.var(x) / np.mean(x), 'range': lambda x: np.ptp(x), 'level': lambda x: np.mean(x),
    'max': lambda x: np.max(x), 'variance': lambda x: np.var(x), 'median': lambda x: np.median(x),
    'poisson': lambda x: np.sqrt(np.mean(x)), 'l2-norm': lambda x: np.sqrt(np.sum(x * x)),
    'vast_2': lambda x: np.var(x) * _kurt(x) ** 2 / np.mean(x), 'vast_3': lambda x: np.var(x) * _kurt(x) ** 2 / np.max(x),
    'vast_4': lambda x: np.var(x) * _kurt(x) ** 2 / np.ptp(x),
}


def _kurt(x):
    c = x - np.mean(x)
    return np.mean(c ** 4) / np.mean(c ** 2) ** 2 - 3


@pytest.mark.parametrize('scale_type', sorted(SCALINGS))
def test_scale_gpr_data(scale_type):
    X, F, P = field_case()
    g = GPR(X, F, None, P, engine=GpNumpyEngine())
    P0 = g.scale_GPR_data(P, scale_type)
    for i in range(P.shape[1]):
        scl = SCALINGS[scale_type](P[:, i])
        assert np.allclose(g.P_scl[:, i], scl, rtol=1e-13) and np.allclose(g.P_cnt[:, i], np.mean(P[:, i]), rtol=1e-15)
        assert np.allclose(P0[:, i], (P[:, i] - np.mean(P[:, i])) / scl, rtol=1e-12, atol=1e-15)


def test_refusals():
    X, F, P = field_case()
    eng = GpNumpyEngine()
    with pytest.raises(Exception) as ei:
        GPR(X, F, None, P[:-1], engine=eng)
    assert type(ei.value) is Exception
    assert str(ei.value) == 'The number of parameters (11) is different from the number of columns of X (12)'
    g = GPR(X, F, None, P, engine=eng)
    with pytest.raises(NotImplementedError) as ei:
        g.scale_GPR_data(P, 'auto')
    assert str(ei.value) == 'The scaling method selected has not been implemented yet'
    with pytest.raises(AttributeError) as ei:
        g.predict(P)
    assert str(ei.value) == 'The function fit has to be called before calling predict.'
    g.fit(select_modes='number', n_modes=2)
    with pytest.raises(AttributeError, match='The function fit has to be called before calling predict.'):
        g.predict(P)                                           # fitted, not trained: the reference's text
    with pytest.raises(AttributeError, match="no attribute 'models'"):
        g.update(P[:1], g.Ar[:1])
    eng.launches = 0
    for kw in (dict(mean='constant'), dict(likelihood=object()), dict(kernel='matern'), dict(kernel=object()),
               dict(kernel='periodic')):
        with pytest.raises(NotImplementedError):
            g.train(**kw)
    for kw in (dict(max_iter=-1), dict(lr=0.0), dict(rel_error=-1.0), dict(lr=np.inf)):
        with pytest.raises(ValueError):
            g.train(**kw)
    mt = GPR(X, F, None, P, gpr_type='MultiTask', engine=eng)
    mt.fit(select_modes='number', n_modes=2)
    with pytest.raises(NotImplementedError, match='MultiTask'):
        mt.train()
    Vr = g.Vr.copy()
    g.Vr = np.where(np.arange(12)[:, None] == 3, np.nan, Vr)
    with pytest.raises(ValueError, match='Vr has entries that are not finite'):
        g.train()
    g.Vr = Vr
    P0 = g.P0.copy()
    g.P0 = np.where(np.arange(12)[:, None] == 0, np.inf, P0)
    with pytest.raises(ValueError, match='P0 has entries that are not finite'):
        g.train()
    g.P0 = P0
    assert eng.launches == 0 and not hasattr(g, 'models')       # every refusal came before any engine call
    g.train(max_iter=5)
    with pytest.raises(NotImplementedError, match='problem_dict'):
        g.predict(P, problem_dict={})
    with pytest.raises(NotImplementedError, match='retrain=True'):
        g.update(P[:1], g.Ar[:1], retrain=True)
    with pytest.raises(ValueError, match='shape'):
        g.predict(np.zeros((2, 3)))
    with pytest.raises(ValueError, match='not finite'):
        g.predict(np.array([[np.nan, 1.0]]))
    with pytest.raises(ValueError, match='A_new must have shape'):
        g.update(P[:2], g.Ar[:1])
    assert g.predict(np.zeros((0, 2)))[0].shape == (0, 2)


def test_more_than_800_points_are_refused():
    rng = np.random.default_rng(0)
    X = rng.standard_normal((6, 801))
    eng = GpNumpyEngine()
    g = GPR(X, 3, None, rng.standard_normal((801, 1)), engine=eng)
    g.fit(select_modes='number', n_modes=2)
    eng.launches = 0
    with pytest.raises(NotImplementedError, match='801 training points exceed the 800'):
        g.train()
    assert eng.launches == 0
    h = fitted(r=2)
    h.train(max_iter=2)
    with pytest.raises(NotImplementedError, match='exceed the 800'):
        h.update(np.ones((800, 2)), np.ones((800, 2)))


def test_engine_without_the_gp_calls_is_refused():
    X, F, P = field_case()
    g = GPR(X, F, None, P, engine=FieldStdNumpyEngine())
    g.fit(select_modes='number', n_modes=2)
    with pytest.raises(NotImplementedError, match='no CPU fallback'):
        g.train()


def test_update_equals_a_fresh_factorisation_of_the_concatenated_data():
    g = fitted()
    g.train(max_iter=60)
    raw = np.stack([q.raw for q in g.models])
    P_new = np.array([[1.7, 333.0], [2.9, 310.0], [3.8, 349.0]])
    A_new = g.predict(P_new)[0] + 0.01 * np.abs(g.Ar).max() * np.random.default_rng(1).standard_normal((3, 3))
    before = g.predict(P_new)[1]
    g.update(P_new, A_new, A_sigma_new=np.ones((3, 3)))
    assert g.Vr_sigma.shape == (15, 3) and np.all(g.Vr_sigma == 0) and g.gpr_info_['n_train'] == 15
    assert g.P0.shape == (12, 2) and all(np.array_equal(q.raw, raw[i]) for i, q in enumerate(g.models))
    P0_tot = np.concatenate([g.P0, (P_new - g.P_cnt[0]) / g.P_scl[0]])
    Y_tot = np.concatenate([g.Vr, A_new / g.Sigma_r])
    D = gp_distance(P0_tot)
    ev = [gp_loss_grad(D, Y_tot[:, i], raw[i], 'matern52') for i in range(3)]
    assert np.allclose(g._d['gp_Kinv'].numpy(), np.stack([e['Kinv'] for e in ev]), rtol=1e-12, atol=1e-12)
    assert np.allclose(g._d['gp_alpha'].numpy(), np.stack([e['alpha'] for e in ev]), rtol=1e-12, atol=1e-12)
    # loss and gradient describe the new data at the kept hyper-parameters; the iteration count still the training
    its = g.gpr_info_['iterations'].copy()
    assert np.allclose(g.gpr_info_['loss'], [e['loss'] for e in ev], rtol=1e-12) and np.allclose(g.gpr_info_['grad'], [e['grad'] for e in ev], rtol=1e-9, atol=1e-13)
    assert [q.loss for q in g.models] == g.gpr_info_['loss'].tolist() and np.array_equal(its, [q.iterations for q in g.models])
    P_star = np.array([[2.0, 330.0], [1.7, 333.0]])
    mean, var = gp_predict(P0_tot, (P_star - g.P_cnt[0]) / g.P_scl[0], raw, np.stack([e['Kinv'] for e in ev]),
                           np.stack([e['alpha'] for e in ev]), 'matern52')
    A_pred, A_sigma = g.predict(P_star)
    assert np.allclose(A_pred, mean * g.Sigma_r, rtol=1e-12, atol=1e-14) and np.allclose(A_sigma, np.sqrt(var) * g.Sigma_r, rtol=1e-12)
    assert np.all(g.predict(P_new)[1] < before)                # data at a point lowers the uncertainty there


def test_pickle_round_trip():
    g = fitted()
    g.train(max_iter=30)
    P_star = np.array([[2.2, 320.0], [3.3, 341.0]])
    want = g.predict(P_star)
    blob = pickle.dumps(g)
    h = pickle.loads(blob)
    assert all(isinstance(v, np.ndarray) for v in h._d.stash.values()) and set(h._d.stash) >= {'gp_P0', 'gp_Y', 'gp_raw', 'gp_Kinv', 'gp_alpha'}
    h._eng = GpNumpyEngine()
    got = h.predict(P_star)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert [q.raw.tolist() for q in h.models] == [q.raw.tolist() for q in g.models] and h.kernel == 'matern52'
    assert np.array_equal(h.reconstruct_std(got[1]), g.reconstruct_std(want[1]))
    # a new fit drops the trained state
    h.fit(select_modes='number', n_modes=2)
    assert not hasattr(h, 'models') and 'gp_Kinv' not in h._d


def test_package_exports_the_module():
    import openmeasure_amd
    assert 'gpr' in openmeasure_amd.__all__
    from openmeasure_amd import gpr
    assert gpr.GPR is GPR
