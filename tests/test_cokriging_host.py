"""CoKriging on the CPU: the NumPy oracle of the level model (ck_loss_grad, ck_train, ck_predict, ck_two_level -- what
csrc/cokriging.hip is held to in tests/test_cokriging_gpu.py), its gradient against central differences, its reduction to the
plain RBF GP oracle of tests/test_gpr_host.py, and the public class over a NumPy double of the two engine calls.

The model (openmeasure_amd/cokriging.py), per latent dimension: theta = 10^v, u_c = x_ic - x_jc, s_ij = sum_c theta_c u_c^2
coordinate by coordinate, R = exp(-s) + nugget I, F = [rho,] 1 [, X], G = F^T R^-1 F, beta = G^-1 F^T R^-1 y,
gamma = R^-1 (y - F beta), sigma2 = (y - F beta).gamma / (n - P), loss = [(n - P) log sigma2 + log det R] / n; with
W = R^-1 - gamma gamma^T / sigma2: d loss / d v_c = ln10 sum W o (-theta_c u_c^2 exp(-s)) / n.  Adam with beta = (0.9, 0.999),
eps = 1e-8, bias correction, the loop of tests/test_gpr_host.py, v clipped to [v_lo, v_hi] after every step.

Central differences in longdouble with h = 1e-5: truncation h^2 f''' / 6 ~ 1e-11 times a derivative of order one, rounding
2^-64 |f| / h ~ 1e-14; the gradient check asks for 1e-7 max(1, |g|), as tests/test_gpr_ard_host.py does."""
import numpy as np
import pytest
import torch

from openmeasure_amd.cokriging import CKRecord, CoKriging
from openmeasure_amd.rom import DeviceMatrix
from tests.test_field_std_host import FieldStdNumpyEngine
from tests.test_gpr_host import chol_lower, gp_distance, gp_loss_grad, softplus, tri_inv_lower

LD = np.longdouble
DEFAULTS = dict(nugget=1e-10, v_lo=-5.0, v_hi=float(np.log10(50.0)), lr=0.1, max_iter=1000, tol=1e-6)


# ------------------------------------------------------------------------------------------------ the oracle
def ck_trend(X, regr, rho=None):
    """F = [rho,] 1 [, X] in X's dtype"""
    cols = ([] if rho is None else [np.asarray(rho, dtype=X.dtype)[:, None]]) + [np.ones((len(X), 1), dtype=X.dtype)]
    return np.concatenate(cols + ([X] if regr == 'linear' else []), axis=1)


def ck_sqdist(Xa, Xb, theta):
    """s = sum_c (theta_c u_c) u_c, u_c = Xa[:, c] - Xb[:, c] (the difference before the scaling), summed coordinate by
    coordinate; -> s, tu2 (d, a, b) = theta_c u_c^2"""
    tu2 = []
    for c in range(Xa.shape[1]):
        u = Xa[:, c][:, None] - Xb[:, c][None, :]
        tu2.append((theta[c] * u) * u)
    tu2 = np.stack(tu2)
    s = np.zeros(tu2.shape[1:], dtype=Xa.dtype)
    for c in range(len(tu2)):
        s = s + tu2[c]
    return s, tu2


def ck_loss_grad(X, y, v, regr='linear', rho=None, nugget=1e-10, dtype=np.float64, route='chol'):
    """-> dict(loss, grad (d,), Rinv, RinvF, Ginv, beta, gamma, sigma2, R, Rc, G, F, res, logdiag, tu2, theta, W) at v = log10 theta.
    route 'chol': Cholesky factor, its inverse, R^-1 = X^T X; 'inv': numpy.linalg.inv and slogdet (LU; float64 only)."""
    T = np.dtype(dtype).type
    X, y, v = np.asarray(X, dtype=dtype), np.asarray(y, dtype=dtype), np.asarray(v, dtype=dtype)
    n, d = X.shape
    theta = T(10) ** v
    s, tu2 = ck_sqdist(X, X, theta)
    Rc = np.exp(-s)
    R = Rc + T(nugget) * np.eye(n, dtype=dtype)
    if route == 'chol':
        Lc = np.linalg.cholesky(R) if dtype == np.float64 else chol_lower(R)
        Xi = tri_inv_lower(Lc)
        Rinv = Xi.T @ Xi
        logdiag = 2 * np.log(np.diag(Lc))
        logdet = np.sum(logdiag)
    else:
        Rinv, logdet, logdiag = np.linalg.inv(R), np.linalg.slogdet(R)[1], None
    F = ck_trend(X, regr, rho)
    P = F.shape[1]
    RinvF = Rinv @ F
    G = F.T @ RinvF
    b = RinvF.T @ y
    Lg = chol_lower(G)
    if not np.all(np.isfinite(Lg)):
        raise np.linalg.LinAlgError('the trend matrix is not positive definite')
    Li = tri_inv_lower(Lg)
    Ginv = Li.T @ Li
    beta = Li.T @ (Li @ b)
    res = y - F @ beta
    gamma = Rinv @ res
    sigma2 = res @ gamma / (n - P)
    loss = ((n - P) * np.log(sigma2) + logdet) / n
    W = Rinv - np.outer(gamma, gamma) / sigma2
    grad = np.array([np.log(T(10)) * np.sum(W * (-tu2[c] * Rc)) / n for c in range(d)], dtype=dtype)
    return dict(loss=loss, grad=grad, Rinv=Rinv, RinvF=RinvF, Ginv=Ginv, beta=beta, gamma=gamma, sigma2=sigma2, R=R, Rc=Rc, G=G,
                F=F, res=res, logdiag=logdiag, tu2=tu2, theta=theta, W=W)


def ck_train(X, y, regr='linear', rho=None, v0=None, nugget=1e-10, v_lo=-5.0, v_hi=float(np.log10(50.0)), lr=0.1, max_iter=1000,
             tol=1e-6, dtype=np.float64, route='chol'):
    """The training loop of one model.  -> dict(v (after the last step), iterations, loss, e (of the last evaluation), es (every
    e), trace (iterations, 1 + d) = (loss, v) per evaluation)"""
    T = np.dtype(dtype).type
    d = X.shape[1]
    p = np.full(d, np.log10(0.5), dtype=dtype) if v0 is None else np.array(v0, dtype=dtype)
    m1, m2 = np.zeros(d, dtype=dtype), np.zeros(d, dtype=dtype)
    b1, b2, b1t, b2t = T(0.9), T(0.999), T(1), T(1)
    loss_old, e, j, trace, es, loss = T(1e10), T(1e10), 0, [], [], T(np.nan)
    while e > tol and j < max_iter:
        ev = ck_loss_grad(X, y, p, regr, rho, nugget, dtype, route)
        loss, g = ev['loss'], ev['grad']
        e = abs(loss - loss_old)
        loss_old = loss
        es.append(e)
        trace.append(np.concatenate([[loss], p]))
        b1t, b2t = b1t * b1, b2t * b2
        m1 = b1 * m1 + (1 - b1) * g
        m2 = b2 * m2 + (1 - b2) * g * g
        p = np.clip(p - (T(lr) / (1 - b1t)) * (m1 / (np.sqrt(m2) / np.sqrt(1 - b2t) + T(1e-8))), T(v_lo), T(v_hi))
        j += 1
    return dict(v=p, iterations=j, loss=loss, e=e, es=np.array(es, dtype=dtype), trace=np.array(trace, dtype=dtype).reshape(-1, 1 + d))


def ck_predict(X, Xs, v, ev, regr='linear', rho_star=None):
    """mean and own mean squared error of the model evaluated as ``ev`` = ck_loss_grad(...) at v -> two (n_p,) arrays"""
    dt = ev['Rinv'].dtype
    X, Xs, v = np.asarray(X, dtype=dt), np.asarray(Xs, dtype=dt), np.asarray(v, dtype=dt)
    rs = np.exp(-ck_sqdist(Xs, X, dt.type(10) ** v)[0])
    fs = ck_trend(Xs, regr, rho_star)
    mean = fs @ ev['beta'] + rs @ ev['gamma']
    u = rs @ ev['RinvF'] - fs
    mse = ev['sigma2'] * (1 - np.einsum('pi,ij,pj->p', rs, ev['Rinv'], rs) + np.einsum('pa,ab,pb->p', u, ev['Ginv'], u))
    return mean, np.maximum(mse, 0)


def ck_two_level(X0, n_u, ev0, v0, ev1, v1, Xs, regr='linear'):
    """Le Gratiet's recursion over two trained levels (level 1 on X0[n_u:]) -> mu, MSE at Xs"""
    m0, s0 = ck_predict(X0, Xs, v0, ev0, regr)
    m1, s1 = ck_predict(X0[n_u:], Xs, v1, ev1, regr, rho_star=m0)
    srho2 = ev1['beta'][0] ** 2 + ev1['sigma2'] * ev1['Ginv'][0, 0]
    return m1, srho2 * s0 + s1


def ck_case(n, d, r, seed=0, noise=0.05, spread=1.0):
    """parameters X (n, d) = spread x standard normal, smooth targets Y (n, r) of unit variance with a little noise, and a column
    per target that is correlated with it (what the lower level's data is to the upper level's): rho (n, r)"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    Y, rho = np.empty((n, r)), np.empty((n, r))
    for q in range(r):
        w = rng.standard_normal(d)
        base = np.sin((q % 3 + 1) * 0.7 * (X @ w) + q) + 0.3 * (X @ rng.standard_normal(d))
        Y[:, q] = base + noise * rng.standard_normal(n)
        rho[:, q] = 0.6 * base + 0.3 * np.cos(X @ rng.standard_normal(d)) + noise * rng.standard_normal(n)
    Y = (Y - Y.mean(axis=0)) / np.maximum(Y.std(axis=0), 1e-300)
    return X * spread, Y, rho


# ------------------------------------------------------------------------------------------------ the engine double
class CkNumpyEngine(FieldStdNumpyEngine):
    """NumpyEngine + the two co-kriging calls with the contract of HipEngine's, computed by the oracle"""

    CK_REGR = {'constant': 0, 'linear': 1}
    CK_FIT_KEYS = ('Rinv', 'RinvF', 'Ginv', 'beta', 'gamma', 'sigma2')

    @staticmethod
    def ck_n_trend(d, regr, rho):
        return (1 if rho else 0) + 1 + (d if regr == 'linear' else 0)

    def ck_train(self, X, Y, rho, regr, v, nugget, v_lo, v_hi, lr, max_iter, tol, trace=False):
        Xn, Yn, vn = X.numpy(), Y.numpy(), v.numpy().copy()
        rn = None if rho is None else rho.numpy()
        n, d = Xn.shape
        r = Yn.shape[1]
        P = self.ck_n_trend(d, regr, rho is not None)
        assert vn.shape == (r, d) and n > P
        fit = dict(Rinv=np.empty((r, n, n)), RinvF=np.empty((r, n, P)), Ginv=np.empty((r, P, P)), beta=np.empty((r, P)),
                   gamma=np.empty((r, n)), sigma2=np.empty(r))
        info = np.zeros((r, 4 + d))
        tr = np.zeros((r, max_iter, 1 + d)) if trace and max_iter > 0 else None
        self.launches = getattr(self, 'launches', 0) + 1
        self.__dict__.setdefault('calls', []).append(('ck_train', regr, rho is not None, n, max_iter))
        for q in range(r):
            rq, yq = (None if rn is None else np.ascontiguousarray(rn[:, q])), np.ascontiguousarray(Yn[:, q])
            if not np.all(np.isfinite(vn[q])):
                info[q, 3] = 2                                   # the first pivot of R is not finite
                continue
            try:
                if max_iter > 0:
                    t = ck_train(Xn, yq, regr, rq, vn[q], nugget, v_lo, v_hi, lr, max_iter, tol)
                    vn[q] = t['v']
                    info[q, :3] = t['iterations'], t['loss'], t['e']
                    info[q, 4:] = ck_loss_grad(Xn, yq, t['trace'][-1, 1:], regr, rq, nugget)['grad']
                    if tr is not None:
                        tr[q, :t['iterations']] = t['trace']
                ev = ck_loss_grad(Xn, yq, vn[q], regr, rq, nugget)
            except np.linalg.LinAlgError:
                info[q, 3] = 1
                continue
            if not (np.isfinite(ev['loss']) and ev['sigma2'] > 0):
                info[q, 3] = 2 if not np.all(np.isfinite(ev['R'])) else 4
                continue
            for k in self.CK_FIT_KEYS:
                fit[k][q] = ev[k]
            if max_iter == 0:
                info[q, 1], info[q, 4:] = ev['loss'], ev['grad']
        f = torch.from_numpy
        return f(vn), {k: f(a) for k, a in fit.items()}, f(info), None if tr is None else f(tr)

    def ck_predict(self, X, Xstar, rho_star, regr, v, fit):
        self.launches = getattr(self, 'launches', 0) + 1
        self.__dict__.setdefault('calls', []).append(('ck_predict', regr, rho_star is not None, len(Xstar)))
        vn = v.numpy()
        r = len(vn)
        mean, mse = np.empty((len(Xstar), r)), np.empty((len(Xstar), r))
        for q in range(r):
            ev = {k: fit[k][q].numpy() for k in self.CK_FIT_KEYS}
            mean[:, q], mse[:, q] = ck_predict(X.numpy(), Xstar.numpy(), vn[q], ev, regr,
                                               None if rho_star is None else rho_star.numpy()[:, q])
        return torch.from_numpy(mean), torch.from_numpy(mse)


# ------------------------------------------------------------------------------------------------ a two-mesh case
def lf_fn(s, x, f):
    return (f + 1) * (np.sin(np.outer(s, 1.0 + 0.5 * x[:, 0]) + f) + 0.4 * np.outer(s * s, x[:, 1]))


def hf_fn(s, x, f):
    return 1.6 * lf_fn(s, x, f) + 0.5 * np.outer(np.cos(2 * s), x[:, 1] ** 2) + 0.2 * np.outer(s, np.sin(3 * x[:, 0]))


def two_mesh_case(n_u=14, n_l=8, seed=4, noise=1e-3):
    """d = 2 parameters; LF on 40 points x 2 features (80 rows), HF on 67 points x 2 features (134 rows) -> dict of the
    constructor's arguments"""
    rng = np.random.default_rng(seed)
    X_u, X_l = rng.uniform(-1, 1, (n_u, 2)), rng.uniform(-1, 1, (n_l, 2))
    s_lf, s_hf = np.linspace(0, 1, 40), np.linspace(0, 1, 67) ** 1.3
    lf = lambda x: np.concatenate([lf_fn(s_lf, x, f) + 3 * f for f in range(2)])
    hf = lambda x: np.concatenate([hf_fn(s_hf, x, f) + 3 * f for f in range(2)])
    Y_lf_l, Y_lf_u, Y_hf_l = lf(X_l), lf(X_u), hf(X_l)
    return dict(X_train_l=X_l, X_train_u=X_u, Y_train_lf_l=Y_lf_l + noise * rng.standard_normal(Y_lf_l.shape),
                Y_train_lf_u=Y_lf_u + noise * rng.standard_normal(Y_lf_u.shape),
                Y_train_hf_l=Y_hf_l + noise * rng.standard_normal(Y_hf_l.shape), xyz_lf=None, xyz_hf=None, n_features=2), hf


def built(engine=None, r_hf=3, r_lf=3, **kw):
    args, hf = two_mesh_case(**kw)
    ck = CoKriging(**args, engine=engine or CkNumpyEngine())
    ck.manifold_alignment(select_modes='number', n_modes_hf=r_hf, n_modes_lf=r_lf)
    return ck, args, hf


# ------------------------------------------------------------------------------------------------ tests: the oracle
@pytest.mark.parametrize('d', [1, 3])
@pytest.mark.parametrize('regr,with_rho', [('linear', False), ('linear', True), ('constant', False), ('constant', True)])
def test_oracle_gradient_against_central_differences(regr, with_rho, d):
    X, Y, rho = ck_case(14, d, 1, seed=5 + d)
    rq = rho[:, 0] if with_rho else None
    for v0, nugget in ((-0.3, 1e-3), (0.4, 1e-10), (-1.2, 1e-6)):
        v = (v0 + 0.25 * np.arange(d)).astype(LD)
        g = ck_loss_grad(X, Y[:, 0], v, regr, rq, nugget, dtype=LD)['grad']
        assert g.shape == (d,) and g.dtype == LD
        for c in range(d):
            h = np.zeros(d, dtype=LD)
            h[c] = LD(1e-5)
            num = (ck_loss_grad(X, Y[:, 0], v + h, regr, rq, nugget, dtype=LD)['loss']
                   - ck_loss_grad(X, Y[:, 0], v - h, regr, rq, nugget, dtype=LD)['loss']) / (2 * h[c])
            assert abs(num - g[c]) <= 1e-7 * max(1, abs(g[c])), (regr, with_rho, d, v0, c, float(num), float(g[c]))


@pytest.mark.parametrize('d', [1, 3])
def test_constant_trend_without_rho_has_the_plain_rbf_inverse(d):
    """regr='constant', no rho column, equal theta: R is the RBF kernel matrix of tests/test_gpr_host.py at l = 1 / sqrt(2 theta)
    with the noise s2 as the nugget, so R^-1 is that oracle's K^-1 (to 1e-11 of its largest entry: kappa(K) ~ 1e2 here)."""
    X, Y, _ = ck_case(15, d, 1, seed=9 + d)
    D = gp_distance(X)
    for raw_l, raw_n in ((0.0, -3.0), (0.8, -2.0), (-0.5, -4.0)):
        old = gp_loss_grad(D, Y[:, 0], np.array([raw_l, raw_n, 0.0]), 'rbf')
        ell, s2 = softplus(np.float64(raw_l)), softplus(np.float64(raw_n)) + 1e-4
        new = ck_loss_grad(X, Y[:, 0], np.full(d, np.log10(1 / (2 * ell * ell))), 'constant', None, nugget=s2)
        assert np.max(np.abs(new['Rinv'] - old['Kinv'])) <= 1e-11 * np.max(np.abs(old['Kinv']))
        assert new['F'].shape == (15, 1) and new['Ginv'].shape == (1, 1)
        # beta is the generalised least-squares mean, gamma the plain oracle's alpha at that mean
        mu = np.sum(old['Kinv'] @ Y[:, 0]) / np.sum(old['Kinv'])
        assert abs(new['beta'][0] - mu) <= 1e-11 * max(1, abs(mu))
        assert np.max(np.abs(new['gamma'] - old['Kinv'] @ (Y[:, 0] - mu))) <= 1e-10 * np.max(np.abs(new['gamma']))


def test_oracle_training_loop_clips_and_predicts():
    X, Y, rho = ck_case(20, 2, 1, seed=2)
    t = ck_train(X, Y[:, 0], 'linear', rho[:, 0], max_iter=7, tol=0.0, nugget=1e-3)
    assert t['iterations'] == 7 and t['trace'].shape == (7, 3) and np.all(t['trace'][0, 1:] == np.log10(0.5))
    assert np.allclose(np.abs(t['trace'][1, 1:] - t['trace'][0, 1:]), 0.1, rtol=1e-4)   # Adam's first step is lr g / (|g| + 1e-8)
    c = ck_train(X, Y[:, 0], 'linear', None, v0=[0.2, 0.2], max_iter=5, tol=0.0, nugget=1e-3, v_lo=0.1, v_hi=0.25)
    tr = c['trace'][:, 1:]
    assert np.all((tr >= 0.1) & (tr <= 0.25)) and np.any((tr[1:] == 0.25) | (tr[1:] == 0.1))        # a first step of 0.1 leaves the box
    ev = ck_loss_grad(X, Y[:, 0], t['v'], 'linear', rho[:, 0], 1e-3)
    Xs = np.stack([X[4], X.mean(axis=0) + 1000.0])
    rs = np.array([rho[4, 0], 0.3])
    mean, mse = ck_predict(X, Xs, t['v'], ev, 'linear', rs)
    fs = ck_trend(Xs, 'linear', rs)
    assert abs(mean[1] - fs[1] @ ev['beta']) <= 1e-12 * np.sum(np.abs(fs[1] * ev['beta']))       # far away: the trend alone
    assert abs(mse[1] - ev['sigma2'] * (1 + fs[1] @ ev['Ginv'] @ fs[1])) <= 1e-12 * mse[1]
    assert abs(mean[0] - Y[4, 0]) <= 2e-3 * np.max(np.abs(ev['gamma'])) and mse[0] <= 4e-3 * ev['sigma2']   # a training point


def prototype_case():
    """the smooth noise-free two-fidelity pair of functions, 40 unlinked + 12 linked points, 200 held out (fixed seed)"""
    rng = np.random.default_rng(0)
    d, nl, nu = 2, 12, 40
    f_lf = lambda x: np.sin(3 * x[:, 0]) + 0.5 * np.cos(2 * x[:, 1]) + 0.3 * x[:, 0]
    f_hf = lambda x: 1.7 * f_lf(x) + 0.4 * x[:, 1] ** 2 - 0.2 + 0.15 * np.sin(5 * x[:, 0] * x[:, 1])
    Xu, Xl, Xt = rng.uniform(-1, 1, (nu, d)), rng.uniform(-1, 1, (nl, d)), rng.uniform(-1, 1, (200, d))
    return Xu, Xl, Xt, f_lf, f_hf


def test_cokriging_beats_kriging_of_the_hf_points_alone():
    """The statistical claim, oracle alone, CPU only: on the prototype's case co-kriging's RMSE over 200 held-out points is below
    half that of a universal kriging of the 12 HF points alone.  Measured with this oracle: 0.138 against 0.433 (levels
    converged after 110 and 90 evaluations, HF alone after 87)."""
    Xu, Xl, Xt, f_lf, f_hf = prototype_case()
    nu = len(Xu)
    X0 = np.vstack([Xu, Xl])
    mu, sd = X0.mean(0), X0.std(0)
    y0, y1 = f_lf(X0), f_hf(Xl)
    yb = np.concatenate([y0[:nu], y1])
    ym, ys = yb.mean(), yb.std()
    X0n, Xtn, y0n, y1n = (X0 - mu) / sd, (Xt - mu) / sd, (y0 - ym) / ys, (y1 - ym) / ys
    ta = ck_train(X0n, y0n)
    tb = ck_train(X0n[nu:], y1n, rho=y0n[nu:])
    th = ck_train(X0n[nu:], y1n)
    assert max(ta['iterations'], tb['iterations'], th['iterations']) < 1000                      # all three converged
    ea, eb = ck_loss_grad(X0n, y0n, ta['v']), ck_loss_grad(X0n[nu:], y1n, tb['v'], rho=y0n[nu:])
    m, mse = ck_two_level(X0n, nu, ea, ta['v'], eb, tb['v'], Xtn)
    mh, _ = ck_predict(X0n[nu:], Xtn, th['v'], ck_loss_grad(X0n[nu:], y1n, th['v']))
    truth = f_hf(Xt)
    rmse_ck, rmse_hf = np.sqrt(np.mean((m * ys + ym - truth) ** 2)), np.sqrt(np.mean((mh * ys + ym - truth) ** 2))
    print(f'co-kriging RMSE {rmse_ck:.3f} ({ta["iterations"]} + {tb["iterations"]} evaluations), HF alone {rmse_hf:.3f} '
          f'({th["iterations"]}); mean predicted std {np.sqrt(mse.mean()) * ys:.3f}')
    assert rmse_ck < 0.5 * rmse_hf
    assert np.all(mse >= 0) and np.all(np.isfinite(mse))


# ------------------------------------------------------------------------------------------------ tests: the class
def reference_alignment(args, r_hf, r_lf):
    """reference cokriging.py:56-102 restated with numpy.linalg.svd ('std' scaling, select_modes='number')"""
    def scale(Y, F):
        n_pts = Y.shape[0] // F
        X0 = np.empty_like(Y)
        for f in range(F):
            x = Y[f * n_pts:(f + 1) * n_pts]
            X0[f * n_pts:(f + 1) * n_pts] = (x - np.average(x, axis=1)[:, None]) / np.std(x)
        return X0
    F, n_l = args['n_features'], args['X_train_l'].shape[0]
    X0_hf = scale(args['Y_train_hf_l'], F)
    X0_lf = scale(np.concatenate((args['Y_train_lf_l'], args['Y_train_lf_u']), axis=1), F)
    U_hf, S_hf, V_hf = np.linalg.svd(X0_hf, full_matrices=False)
    U_lf, S_lf, V_lf = np.linalg.svd(X0_lf, full_matrices=False)
    Zr_hf, Zr_lf = (np.diag(S_hf) @ V_hf)[:r_hf], (np.diag(S_lf) @ V_lf)[:r_lf]
    if r_lf < r_hf:
        Zr_lf = np.concatenate([Zr_lf, np.zeros((r_hf - r_lf, Zr_lf.shape[1]))], axis=0)
    Zr_lf_l = Zr_lf[:, :n_l]
    Z0r_hf = Zr_hf - Zr_hf.mean(axis=1, keepdims=True)
    Z0r_lf_l = Zr_lf_l - Zr_lf_l.mean(axis=1, keepdims=True)
    Ur, Sigmar, Vr_t = np.linalg.svd(Z0r_lf_l @ Z0r_hf.T, full_matrices=False)
    sr = np.sum(Sigmar) / np.trace(Z0r_lf_l @ Z0r_lf_l.T)
    Qr = Vr_t.T @ Ur.T
    return dict(Zr_aligned=sr * Qr @ Zr_lf, sr=sr, Qr=Qr, Zr_hf=Zr_hf, S_hf=S_hf, S_lf=S_lf, U_hf=U_hf[:, :r_hf])


@pytest.mark.parametrize('r_hf,r_lf', [(4, 2), (2, 4), (3, 3)])
def test_manifold_alignment_against_the_reference_lines(r_hf, r_lf):
    """Sign-invariant quantities only (a POD mode's sign is the eigensolver's): |Zr_aligned| and |Zr_hf| row by row, sr, |Qr|.
    The scores come from a Gram-route eigensolve: 1e-8 relative to the largest score (rom.py: as good as LAPACK's to ~1e-8)."""
    ck, args, _ = built(r_hf=r_hf, r_lf=r_lf)
    ref = reference_alignment(args, r_hf, r_lf)
    assert (ck.r_hf, ck.r_lf, ck.n_latent) == (r_hf, r_lf, r_hf)
    assert ck.Zr_aligned.shape == (r_hf, 22) and ck.Zr_hf.shape == (r_hf, 8) and ck.Qr.shape == (r_hf, max(r_hf, r_lf))
    tol = 1e-8
    assert abs(ck.sr - ref['sr']) <= tol * ref['sr']
    assert np.max(np.abs(np.abs(ck.Qr) - np.abs(ref['Qr']))) <= tol
    for k in range(r_hf):
        s = np.sign(np.sum(ck.Zr_hf[k] * ref['Zr_hf'][k]))
        assert np.max(np.abs(s * ck.Zr_hf[k] - ref['Zr_hf'][k])) <= tol * np.max(np.abs(ref['Zr_hf']))
        assert np.max(np.abs(s * ck.Zr_aligned[k] - ref['Zr_aligned'][k])) <= tol * np.max(np.abs(ref['Zr_aligned']))
    assert np.allclose(ck.Sigma_hf[:r_hf], ref['S_hf'][:r_hf], rtol=1e-8) and np.allclose(ck.Sigma_lf[:r_lf], ref['S_lf'][:r_lf], rtol=1e-8)
    Ur = ck.Ur_hf
    assert isinstance(Ur, torch.Tensor) and tuple(Ur.shape) == (134, r_hf)                      # the basis stays a device tensor
    assert np.max(np.abs(np.abs(Ur.numpy()) - np.abs(ref['U_hf']))) <= 1e-7


def test_fit_predict_through_the_engine_double():
    eng = CkNumpyEngine()
    ck, args, hf = built(eng)
    ck.max_iter = 40
    ck.fit()
    assert [c[:3] for c in eng.calls] == [('ck_train', 'linear', False), ('ck_train', 'linear', True)]
    assert eng.calls[0][3:] == (22, 40) and eng.calls[1][3:] == (8, 40)
    info = ck.cokriging_info_
    assert len(ck.model_list) == 3 and all(isinstance(m, CKRecord) for m in ck.model_list)
    for lev, P in ((0, 3), (1, 4)):
        assert info['theta'][lev].shape == (3, 2) and info['beta'][lev].shape == (3, P) and info['sigma2'][lev].shape == (3,)
        assert info['iterations'][lev].shape == info['loss'][lev].shape == info['status'][lev].shape == (3,)
        assert np.all(info['status'][lev] == 0) and np.all(info['theta'][lev] >= 1e-5) and np.all(info['theta'][lev] <= 50 * (1 + 1e-15))
    assert info['rho'][0] is None and np.array_equal(info['rho'][1], info['beta'][1][:, 0])
    # level by level the numbers are the oracle's on the class's own normalised data
    X = np.concatenate([args['X_train_u'], args['X_train_l']])
    Xn = (X - X.mean(axis=0)) / X.std(axis=0)
    Y0 = np.concatenate([ck.Zr_aligned[:, 8:], ck.Zr_aligned[:, :8]], axis=1)
    yb = np.concatenate([Y0[:, :14], ck.Zr_hf], axis=1)
    assert np.array_equal(ck.y_mean, yb.mean(axis=1)) and np.array_equal(ck.y_std, yb.std(axis=1))
    X_test = np.array([[0.1, -0.3], [0.7, 0.6], args['X_train_l'][2]])
    Z_pred, Z_mse = ck.predict_latent(X_test)
    assert Z_pred.shape == Z_mse.shape == (3, 3) and eng.calls[-2][:3] == ('ck_predict', 'linear', False) and eng.calls[-1][2] is True
    for k in range(3):
        y0n, y1n = (Y0[k] - ck.y_mean[k]) / ck.y_std[k], (ck.Zr_hf[k] - ck.y_mean[k]) / ck.y_std[k]
        t0 = ck_train(Xn, y0n, max_iter=40)
        t1 = ck_train(Xn[14:], y1n, rho=y0n[14:], max_iter=40)
        rec = ck.model_list[k]
        # (to 1e-8, not bit for bit: BLAS need not sum operands of another layout in the same order, and 40 steps carry a
        # last bit along)
        assert np.allclose(rec.theta, 10.0 ** np.stack([t0['v'], t1['v']]), rtol=1e-8, atol=0)
        assert rec.iterations.tolist() == [t0['iterations'], t1['iterations']]
        e0, e1 = ck_loss_grad(Xn, y0n, t0['v']), ck_loss_grad(Xn[14:], y1n, t1['v'], rho=y0n[14:])
        assert np.isclose(rec.rho, e1['beta'][0], rtol=1e-8, atol=0) and np.allclose(rec.sigma2, [e0['sigma2'], e1['sigma2']], rtol=1e-8, atol=0)
        m, mse = ck_two_level(Xn, 14, e0, t0['v'], e1, t1['v'], (X_test - X.mean(axis=0)) / X.std(axis=0))
        assert np.allclose(Z_pred[k], m * ck.y_std[k] + ck.y_mean[k], rtol=0, atol=1e-8 * np.max(np.abs(Z_pred[k])))
        assert np.allclose(Z_mse[k], mse * ck.y_std[k] ** 2, rtol=0, atol=1e-8 * np.max(np.abs(Z_mse[k])))
    Y_pred, Y_var = ck.predict(X_test)
    assert Y_pred.shape == Y_var.shape == (134, 3) and np.all(np.isfinite(Y_pred)) and np.all(Y_var >= 0)
    assert np.array_equal(Y_pred, ck.rom_hf.reconstruct(Z_pred.T)) and np.array_equal(Y_var, ck.rom_hf.reconstruct_std(np.sqrt(Z_mse).T) ** 2)
    truth = hf(X_test)
    assert np.sqrt(np.mean((Y_pred - truth) ** 2)) < 0.25 * np.std(truth)                       # it predicts the HF field
    # the device tensors of predict_latent(to_host=False) go straight into reconstruct
    Zd, Md = ck.predict_latent(X_test, to_host=False)
    assert isinstance(Zd, torch.Tensor) and np.array_equal(Zd.numpy(), Z_pred) and np.array_equal(Md.numpy(), Z_mse)
    assert np.array_equal(ck.rom_hf.reconstruct(Zd.T.contiguous()), Y_pred)
    # truncation: the leading dimensions only
    Z2, M2 = ck.predict_latent(X_test, n_truncated=2)
    assert np.array_equal(Z2, Z_pred[:2]) and np.array_equal(M2, Z_mse[:2])
    Y2, V2 = ck.predict(X_test, n_truncated=2)
    A = np.zeros((3, 3))
    A[:, :2] = Z2.T
    assert np.array_equal(Y2, ck.rom_hf.reconstruct(A)) and np.all(V2 <= Y_var * (1 + 1e-12) + 1e-300)


def test_theta_given_means_no_optimisation():
    eng = CkNumpyEngine()
    ck, args, _ = built(eng)
    ck.theta = [0.3, 1.2]
    ck.fit()
    assert [c[4] for c in eng.calls] == [0, 0]
    assert np.allclose(ck.cokriging_info_['theta'][0], [[0.3, 1.2]] * 3, rtol=1e-15) and np.all(ck.cokriging_info_['iterations'][1] == 0)
    assert np.all(np.isfinite(ck.cokriging_info_['loss'][0]))
    ck.theta = ([0.3, 1.2], 2.0)                                                               # one entry per level
    ck.fit()
    assert np.allclose(ck.cokriging_info_['theta'][1], 2.0, rtol=1e-15)


@pytest.mark.parametrize('which,k', [('hf', 0), ('hf', 2), ('lf', 0), ('lf', 1)])
def test_a_modes_sign_changes_nothing(which, k):
    """Flipping the sign of an HF or LF POD mode (basis column and scores) leaves Y_pred and Y_var unchanged to rounding: 1e-9
    relative to the largest entry (60 Adam steps amplify a rounding-level difference in the targets by kappa(R) ~ 1e4 at most
    with nugget 1e-6)."""
    X_test = np.array([[0.1, -0.3], [0.7, 0.6]])
    out = []
    for flip in (False, True):
        ck, _, _ = built()
        ck.max_iter, ck.tol, ck.nugget = 60, 0.0, 1e-6
        if flip:
            rom = ck.rom_hf if which == 'hf' else ck.rom_lf
            s = np.ones(rom.Ar.shape[1])
            s[k] = -1.0
            Ar, Ur = rom.Ar * s, rom.Ur * s
            rom.Ur = Ur
            rom.Ar = Ar
            ck._align()
        ck.fit()
        out.append(ck.predict(X_test) + ck.predict_latent(X_test))
    (Ya, Va, Za, Ma), (Yb, Vb, Zb, Mb) = out
    if which == 'hf':
        assert np.allclose(Zb[k], -Za[k], rtol=0, atol=1e-9 * np.max(np.abs(Za)))                 # the score follows the mode
    assert np.max(np.abs(Ya - Yb)) <= 1e-9 * np.max(np.abs(Ya)) and np.max(np.abs(Va - Vb)) <= 1e-9 * np.max(np.abs(Va))
    assert np.max(np.abs(Ma - Mb)) <= 1e-9 * np.max(np.abs(Ma))


def test_every_lf_target_is_paired_with_its_own_parameters():
    """The pairing fix.  LF data that is an exact function of the parameters: the level-0 predictor at a training point returns
    the aligned score of the snapshot that was computed THERE -- to 2 nugget |gamma|_inf (the interpolation defect of a nugget) plus
    64 n eps kappa(R) |y|_inf of rounding -- while the reference's pairing (scores linked first against parameters unlinked first)
    returns another snapshot's score."""
    eng = CkNumpyEngine()
    ck, args, _ = built(eng, noise=0.0)
    ck.nugget, ck.max_iter = 1e-8, 30
    ck.fit()
    n_u, n_l = 14, 8
    X = np.concatenate([args['X_train_u'], args['X_train_l']])
    s = ck._d
    m0, _ = eng.ck_predict(s['X'], s['X'], None, 'linear', s['v0'], s['fit0'])
    got = (m0.numpy() * ck.y_std + ck.y_mean).T                                                  # (r, n0), rows of X order
    own = np.concatenate([ck.Zr_aligned[:, n_l:], ck.Zr_aligned[:, :n_l]], axis=1)               # the snapshot computed at row j
    Xn = (X - ck.X_mean) / ck.X_std
    for k in range(3):
        y0n = (own[k] - ck.y_mean[k]) / ck.y_std[k]
        ev = ck_loss_grad(Xn, y0n, s['v0'].numpy()[k], nugget=1e-8)
        bar = (2 * 1e-8 * np.max(np.abs(ev['gamma'])) + 64 * 22 * 2.0 ** -53 * np.linalg.cond(ev['R']) * np.max(np.abs(y0n))) * ck.y_std[k]
        assert np.max(np.abs(got[k] - own[k])) <= bar, (k, np.max(np.abs(got[k] - own[k])), bar)
        # the reference's pairing: Zr_aligned as it is (linked first) against X (unlinked first)
        wrong = ck.Zr_aligned[k]
        yw = (wrong - ck.y_mean[k]) / ck.y_std[k]
        tw = ck_train(Xn, yw, nugget=1e-8, max_iter=30)
        mw, _ = ck_predict(Xn, Xn, tw['v'], ck_loss_grad(Xn, yw, tw['v'], nugget=1e-8))
        assert np.max(np.abs(mw * ck.y_std[k] + ck.y_mean[k] - own[k])) > 0.1 * np.std(own[k])


def test_inputs_may_be_device_tensors_or_device_matrices():
    args, _ = two_mesh_case()
    eng = CkNumpyEngine()
    a = CoKriging(**args, engine=eng)
    a.manifold_alignment(select_modes='number', n_modes_hf=2, n_modes_lf=2)
    mixed = dict(args, Y_train_lf_l=torch.from_numpy(args['Y_train_lf_l']), Y_train_lf_u=DeviceMatrix(torch.from_numpy(args['Y_train_lf_u'])),
                 Y_train_hf_l=DeviceMatrix(torch.from_numpy(args['Y_train_hf_l'])))
    b = CoKriging(**mixed, engine=eng)
    b.manifold_alignment(select_modes='number', n_modes_hf=2, n_modes_lf=2)
    assert np.array_equal(a.Zr_aligned, b.Zr_aligned) and tuple(b._d['Y_lf'].shape) == (80, 22)
    lf = b._d['Y_lf']
    b.manifold_alignment(select_modes='number', n_modes_hf=3, n_modes_lf=2)
    assert b._d['Y_lf'] is lf and b.n_latent == 3                                               # concatenated once


def test_refusals():
    args, _ = two_mesh_case()
    for key, cols in (('Y_train_lf_l', 7), ('Y_train_hf_l', 9), ('Y_train_lf_u', 13)):
        with pytest.raises(ValueError, match='conditions does not correspond'):
            CoKriging(**dict(args, **{key: args[key][:, :cols] if cols < args[key].shape[1] else np.zeros((args[key].shape[0], cols))}))
    with pytest.raises(NotImplementedError, match='sharded'):
        CoKriging(**args, shard=object())
    eng = CkNumpyEngine()
    ck = CoKriging(**args, engine=eng)
    with pytest.raises(AttributeError, match='manifold_alignment'):
        ck.fit()
    ck.manifold_alignment(select_modes='number', n_modes_hf=2, n_modes_lf=2)
    with pytest.raises(AttributeError, match='fit has to be called'):
        ck.predict(np.zeros((1, 2)))
    eng.launches = 0
    for attr, val, exc, text in (('regr_type', 'quadratic', NotImplementedError, 'regr_type'), ('rho_regr', 'linear', NotImplementedError, 'rho_regr'),
                                 ('lr', 0.0, ValueError, 'lr'), ('tol', -1.0, ValueError, 'tol'), ('nugget', float('nan'), ValueError, 'nugget'),
                                 ('thetaL', 60.0, ValueError, 'thetaL'), ('theta0', -1.0, ValueError, 'positive'), ('max_iter', -1, ValueError, 'max_iter')):
        old = getattr(ck, attr)
        setattr(ck, attr, val)
        with pytest.raises(exc, match=text):
            ck.fit()
        setattr(ck, attr, old)
    assert eng.launches == 0 and not hasattr(ck, 'model_list')
    rng = np.random.default_rng(0)
    wide = CoKriging(**dict(args, X_train_l=rng.random((8, 9)), X_train_u=rng.random((14, 9))), engine=eng)
    wide.manifold_alignment(select_modes='number', n_modes_hf=2, n_modes_lf=2)
    with pytest.raises(NotImplementedError, match='9 parameters exceed the 8'):
        wide.fit()
    few = two_mesh_case(n_l=4)[0]
    short = CoKriging(**few, engine=eng)
    short.manifold_alignment(select_modes='number', n_modes_hf=2, n_modes_lf=2)
    with pytest.raises(ValueError, match='more points than trend columns'):
        short.fit()
    short.regr_type = 'constant'                                                                # p' = 1 and 2: four points are enough
    short.max_iter = 3
    short.fit()
    assert short.cokriging_info_['beta'][0].shape == (2, 1) and short.cokriging_info_['beta'][1].shape == (2, 2)
    ck.max_iter = 2
    ck.fit()
    with pytest.raises(ValueError, match='n_truncated'):
        ck.predict_latent(np.zeros((1, 2)), n_truncated=3)
    with pytest.raises(ValueError, match=r'shape \(n_test, 2\)'):
        ck.predict_latent(np.zeros((1, 3)))
    assert eng.launches > 0


def test_more_than_800_points_are_refused():
    rng = np.random.default_rng(0)
    Yl, Yu, Yh = np.zeros((4, 3)), np.zeros((4, 798)), np.zeros((6, 3))
    ck = CoKriging(rng.random((3, 2)), rng.random((798, 2)), Yl, Yu, Yh, None, None, 2, engine=CkNumpyEngine())
    ck.Zr_aligned, ck.Zr_hf, ck.n_latent = np.zeros((1, 801)), np.zeros((1, 3)), 1
    with pytest.raises(NotImplementedError, match='801 training points exceed the 800'):
        ck.fit()


def test_a_failed_factorisation_names_level_dimension_and_nugget():
    eng = CkNumpyEngine()
    args, _ = two_mesh_case()
    args['X_train_u'] = args['X_train_u'].copy()
    args['X_train_u'][1] = args['X_train_u'][0]                                                # a duplicated point, no nugget
    ck = CoKriging(**args, engine=eng)
    ck.manifold_alignment(select_modes='number', n_modes_hf=2, n_modes_lf=2)
    ck.nugget, ck.max_iter = 0.0, 0
    with pytest.raises(np.linalg.LinAlgError, match=r'level 0 \(LF\).*nugget = 0.*dimension 1'):
        ck.fit()


def test_engine_without_the_calls_is_refused():
    ck, _, _ = built(FieldStdNumpyEngine())
    with pytest.raises(NotImplementedError, match="no 'ck_train' .*no CPU fallback"):
        ck.fit()


def test_package_exports_the_module():
    import openmeasure_amd
    assert 'cokriging' in openmeasure_amd.__all__
    from openmeasure_amd import cokriging
    assert cokriging.CoKriging is CoKriging
