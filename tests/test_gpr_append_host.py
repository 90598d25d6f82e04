"""GPR.update(append=True) on the CPU: the NumPy restatement of the append (gp_state_oracle, gp_append_oracle -- what
spr_gp_state_f64 / spr_gp_append_f64 of csrc/gp.hip are held to in tests/test_gpr_append_gpu.py), its algebra against a longdouble
inverse of K', a chain of 40 single-point appends that must not drift, and the public ``GPR.update(append=True)`` /
``GPR.forget`` over a NumPy double of the two engine calls.

The append (include/spr_hip.h), per mode, with K' = [[K, B], [B^T, C]], X = L^-1 of K = L L^T and C including the new points' noise:
    W = X B,  S = C - W^T W = Ls Ls^T (a pivot <= m' eps C_jj is refused),  Z = Ls^-1 W^T X,  N = [-Z, Ls^-1],  X' = [[X, 0], N],
    K'^-1 = [[K^-1, 0], [0, 0]] + N^T N,  logdet' = logdet + 2 sum log diag(Ls),  alpha' = K'^-1 (y' - mu),  the loss of training.

THE BAR is that of tests/test_gpr_gpu.py: rel = 16 m' eps kappa_2(K') with kappa from the longdouble K', times |K'^-1|_2 for K'^-1,
|K'^-1|_2 |res|_2 for alpha, (sa |res| / 2 + sum |log r_jj^2| / 2 + m' log(2 pi) / 2) / m' for the loss and sum |log r_jj^2| for logdet."""
import pickle

import numpy as np
import pytest
import torch

from openmeasure_amd.gpr import GPKernel
from tests.test_gpr_ard_host import fitted2, layout, scaled_t, split, widen
from tests.test_gpr_host import chol_lower, gp_case, gp_kernel, tri_inv_lower
from tests.test_gpr_noise_host import GpNoiseNumpyEngine, gp2_loss_grad_noise

LD = np.longdouble
EPS = 2.0 ** -53
LOG_2PI = np.log(2.0 * np.pi)
F64 = lambda a: np.asarray(a, dtype=np.float64)


# ------------------------------------------------------------------------------------------------ the oracle
def gp_state_oracle(P0, y, raw, kernel, flags, w, v, dtype=np.float64):
    """gp2_loss_grad_noise plus X = L^-1 and logdet -> its dict with X, logdet"""
    ev = gp2_loss_grad_noise(P0, y, raw, kernel, flags, w, v, dtype=dtype)
    K = ev['K']
    ev['X'] = tri_inv_lower(np.linalg.cholesky(K) if dtype == np.float64 else chol_lower(K))
    ev['logdet'] = np.sum(ev['logdiag'])
    return ev


def chol_checked(S, floor=None):
    """chol_lower that refuses a pivot <= floor[j] (0 by default; status 1) or not finite (status 2) as the kernel does"""
    k = len(S)
    L = np.zeros_like(S)
    floor = np.zeros(k, dtype=S.dtype) if floor is None else floor
    for j in range(k):
        p = S[j, j] - L[j, :j] @ L[j, :j]
        if not p > floor[j] or not np.isfinite(p):
            e = np.linalg.LinAlgError(f'pivot {j} of the Schur complement is {float(p)!r}')
            e.status = 2 if not np.isfinite(p) else 1
            raise e
        L[j, j] = np.sqrt(p)
        L[j + 1:, j] = (S[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def gp_append_oracle(P0, y, raw, kernel, flags, w, v, X, Kinv, logdet, k, dtype=np.float64):
    """The formulas of the module docstring for one mode: P0 (m', d), y, w, v (m',), the last k rows new; X, Kinv (m, m) and
    logdet the state of the first m = m' - k rows at raw.  -> dict(X, Kinv, alpha, logdet, loss); LinAlgError with .status."""
    T = np.dtype(dtype).type
    P0, y, raw, w, v = (np.asarray(a, dtype=dtype) for a in (P0, y, raw, w, v))
    X, Kinv = np.asarray(X, dtype=dtype), np.asarray(Kinv, dtype=dtype)
    mp, d = P0.shape
    m = mp - k
    assert 1 <= k < mp and X.shape == Kinv.shape == (m, m)
    ell, o, s2, mu = split(raw, d, flags)
    Z = P0 / ell
    B = o * gp_kernel(kernel, scaled_t(Z[:m], Z[m:])[0])[0]
    C = o * gp_kernel(kernel, scaled_t(Z[m:], Z[m:])[0])[0] + np.diag(w[m:] * s2 + v[m:])
    W = X @ B
    Ls = chol_checked(C - W.T @ W, T(mp * EPS) * np.diag(C))       # a pivot at the size of the cancellation's rounding is not positive
    Lsi = tri_inv_lower(Ls)
    N = np.hstack([-(Lsi @ (W.T @ X)), Lsi])
    X2, Kinv2 = np.zeros((mp, mp), dtype=dtype), np.zeros((mp, mp), dtype=dtype)
    X2[:m, :m], X2[m:] = X, N
    Kinv2[:m, :m] = Kinv
    Kinv2 += N.T @ N
    logdet2 = T(logdet) + 2 * np.sum(np.log(np.diag(Ls)))
    res = y - mu
    alpha = Kinv2 @ res
    return dict(X=X2, Kinv=Kinv2, alpha=alpha, logdet=logdet2, res=res, loss=(res @ alpha / 2 + logdet2 / 2 + mp * T(LOG_2PI) / 2) / mp)


def append_bars(ev_ld, m):
    """rel and the scales of the module docstring from a LONGDOUBLE evaluation of the whole data (gp_state_oracle)"""
    rel = 16 * m * EPS * np.linalg.cond(F64(ev_ld['K']))
    sK = np.linalg.norm(F64(ev_ld['Kinv']), 2)
    rn = np.linalg.norm(F64(ev_ld['res']))
    sl = float(np.sum(np.abs(F64(ev_ld['logdiag']))))
    return rel, dict(Kinv=sK, alpha=sK * rn, logdet=sl, loss=(0.5 * sK * rn * rn + 0.5 * sl + 0.5 * m * LOG_2PI) / m)


def append_errors(got, ev_ld):
    """max absolute differences of an append's outputs (dict with Kinv, alpha, logdet, loss) to the longdouble evaluation"""
    return dict(Kinv=float(np.max(np.abs(got['Kinv'] - ev_ld['Kinv']))), alpha=float(np.max(np.abs(got['alpha'] - ev_ld['alpha']))),
                logdet=float(abs(got['logdet'] - ev_ld['logdet'])), loss=float(abs(got['loss'] - ev_ld['loss'])))


def append_case(m, k, d, r, seed):
    """gp_case over m + k points; noise: every third old point and every other new point carry a given variance (w = 0)"""
    P0, Y = gp_case(m + k, d, r, seed=seed)
    rng = np.random.default_rng(seed + 1)
    w = np.ones(m + k)
    w[2:m:3] = 0.0
    w[m::2] = 0.0
    V = np.where(w[:, None] == 0, (0.15 + 0.3 * rng.random((m + k, r))) ** 2, 0.0)
    return P0, Y, w, V


# ------------------------------------------------------------------------------------------------ tests: the algebra
@pytest.mark.parametrize('m,k,d,flags,kernel', [(1, 1, 1, 0, 'matern52'), (2, 1, 3, 3, 'matern32'), (37, 1, 1, 2, 'matern52'),
                                                (37, 17, 3, 1, 'rbf'), (65, 64, 3, 0, 'matern12'), (130, 2, 3, 3, 'matern52')])
def test_oracle_against_a_longdouble_inverse(m, k, d, flags, kernel):
    P0, Y, w, V = append_case(m, k, d, 1, seed=m + k)
    for s in range(3):
        raw = widen(s, d, flags)
        st = gp_state_oracle(P0[:m], Y[:m, 0], raw, kernel, flags, w[:m], V[:m, 0])
        got = gp_append_oracle(P0, Y[:, 0], raw, kernel, flags, w, V[:, 0], st['X'], st['Kinv'], st['logdet'], k)
        want = gp_state_oracle(P0, Y[:, 0], raw, kernel, flags, w, V[:, 0], dtype=LD)
        rel, sc = append_bars(want, m + k)
        for key, e in append_errors(got, want).items():
            assert e <= rel * sc[key], (key, s, e, rel, sc[key])
        assert np.array_equal(got['X'][:m, :m], st['X']) and np.all(got['X'][:m, m:] == 0) and np.all(np.triu(got['X'], 1) == 0)
        assert np.max(np.abs(got['X'].T @ got['X'] - want['Kinv'])) <= rel * sc['Kinv']


def chain_case(n_steps=40, m=37, seed=11):
    """d = 1, s2 = 1e-4 (raw_n = -40), new points with V = 1e-8 and w = 0, every third one 1e-7 away from an earlier point"""
    rng = np.random.default_rng(seed)
    P0, Y = gp_case(m + n_steps, 1, 1, seed=seed)
    for j in range(0, n_steps, 3):
        src = rng.integers(0, m + j)
        P0[m + j] = P0[src] + 1e-7
        Y[m + j] = Y[src]
    w = np.concatenate([np.ones(m), np.zeros(n_steps)])
    v = np.concatenate([np.zeros(m), np.full(n_steps, 1e-8)])
    return P0, Y[:, 0], w, v, np.array([0.0, -40.0, 0.0])


def test_a_chain_of_forty_single_point_appends_does_not_drift():
    P0, y, w, v, raw = chain_case()
    m, worst = 37, 0.0
    st = gp_state_oracle(P0[:m], y[:m], raw, 'matern52', 0, w[:m], v[:m])
    cur = dict(X=st['X'], Kinv=st['Kinv'], logdet=st['logdet'])
    for n in range(m + 1, m + 41):
        cur = gp_append_oracle(P0[:n], y[:n], raw, 'matern52', 0, w[:n], v[:n], cur['X'], cur['Kinv'], cur['logdet'], 1)
        want = gp_state_oracle(P0[:n], y[:n], raw, 'matern52', 0, w[:n], v[:n], dtype=LD)
        rel, sc = append_bars(want, n)
        for key, e in append_errors(cur, want).items():
            worst = max(worst, e / (rel * sc[key]))
            assert e <= rel * sc[key], (n, key, e, rel, sc[key])
    print(f'chain: worst error / bar {worst:.2e}, final kappa {np.linalg.cond(F64(want["K"])):.2e}')


def test_a_pivot_that_is_not_positive_is_refused_with_its_status():
    S = np.array([[4.0, 2.0], [2.0, 1.0]])
    with pytest.raises(np.linalg.LinAlgError) as e:
        chol_checked(S)
    assert e.value.status == 1
    with pytest.raises(np.linalg.LinAlgError) as e:
        chol_checked(np.array([[np.nan]]))
    assert e.value.status == 2


# ------------------------------------------------------------------------------------------------ the engine double
class GpAppendNumpyEngine(GpNoiseNumpyEngine):
    """GpNoiseNumpyEngine + gp_state / gp_append with the contract of HipEngine's, computed by the oracle; ``launches`` counts
    every call, ``calls`` names them.  ``fail_modes``: modes whose next append reports status 1 (then cleared)."""
    fail_modes = ()

    def gp_state(self, P0, Y, w, V, kernel, flags, raw):
        self._log('gp_state', kernel, flags, len(P0))
        self.launches = getattr(self, 'launches', 0) + 1
        P0n, Yn, wn, Vn, rawn = P0.numpy(), Y.numpy(), w.numpy(), V.numpy(), raw.numpy()
        m, r = Yn.shape
        n_par = layout(P0n.shape[1], flags)[2]
        assert rawn.shape == (r, n_par) and wn.shape == (m,) and Vn.shape == (m, r)
        Kinv, alpha, X = np.empty((r, m, m)), np.empty((r, m)), np.empty((r, m, m))
        info, logdet = np.zeros((r, 4 + n_par)), np.full(r, np.nan)
        for q in range(r):
            try:
                ev = gp_state_oracle(P0n, Yn[:, q], rawn[q], kernel, flags, wn, Vn[:, q])
            except np.linalg.LinAlgError:
                info[q, 3] = 1
                continue
            Kinv[q], alpha[q], X[q], logdet[q] = ev['Kinv'], ev['alpha'], ev['X'], ev['logdet']
            info[q, 1], info[q, 4:] = ev['loss'], ev['grad']
        return tuple(torch.from_numpy(a) for a in (Kinv, alpha, info, X, logdet))

    def gp_append(self, P0, Y, w, V, kernel, flags, raw, X, Kinv, logdet, k):
        self._log('gp_append', kernel, flags, len(P0), k)
        self.launches = getattr(self, 'launches', 0) + 1
        P0n, Yn, wn, Vn, rawn = P0.numpy(), Y.numpy(), w.numpy(), V.numpy(), raw.numpy()
        mp, r = Yn.shape
        assert isinstance(k, int) and 1 <= k <= 64 and mp <= 800 and tuple(X.shape) == tuple(Kinv.shape) == (r, mp - k, mp - k)
        old = [t.numpy().copy() for t in (X, Kinv, logdet)]
        X2, Kinv2, alpha2 = np.full((r, mp, mp), np.nan), np.full((r, mp, mp), np.nan), np.full((r, mp), np.nan)
        logdet2, info = np.full(r, np.nan), np.full((r, 4), np.nan)
        info[:, 0], info[:, 3] = mp, 0
        for q in range(r):
            try:
                if q in self.fail_modes:
                    raise np.linalg.LinAlgError('told to fail')
                ev = gp_append_oracle(P0n, Yn[:, q], rawn[q], kernel, flags, wn, Vn[:, q], old[0][q], old[1][q], old[2][q], k)
            except np.linalg.LinAlgError as e:
                info[q, 3] = getattr(e, 'status', 1)
                continue
            X2[q], Kinv2[q], alpha2[q], logdet2[q] = ev['X'], ev['Kinv'], ev['alpha'], ev['logdet']
            info[q, 1], info[q, 2] = ev['loss'], ev['logdet']
        self.fail_modes = ()
        assert all(np.array_equal(a, t.numpy()) for a, t in zip(old, (X, Kinv, logdet)))       # the old state is never written
        return tuple(torch.from_numpy(a) for a in (X2, Kinv2, alpha2, logdet2, info))


GK = GPKernel('matern52', ard=True, scale=True)
P_STAR = np.array([[2.0, 330.0], [1.7, 333.0], [3.3, 341.0]])


def trained(kernel=None, max_iter=20, eng=None, **kw):
    eng = eng or GpAppendNumpyEngine()
    g = fitted2(eng)
    g.train(kernel=kernel, max_iter=max_iter, **kw)
    return g, eng


def measurements(g, n, seed=1, scale=0.02):
    """n measured points inside the parameter range: the prediction plus a perturbation, standard deviations of that size"""
    rng = np.random.default_rng(seed)
    P = np.column_stack([1.0 + 3.0 * rng.random(n), 300 + 50 * rng.random(n)])
    amax = np.abs(g.Ar).max()
    return P, g.predict(P)[0] + scale * amax * rng.standard_normal((n, 3)), scale * amax * (0.5 + rng.random((n, 3)))


def names(eng, start=0):
    return [c[0] for c in eng.calls[start:] if c[0] != 'gp_predict' and c[0] != 'gp_predict_ard']


def held_bars(g, flags):
    """per mode: rel and scales for the data the object holds now, from the longdouble oracle"""
    P0, Y = g._d['gp_P0'].numpy(), g._d['gp_Y'].numpy()
    w, V = g.gpr_info_['noise_weight'], g.gpr_info_['fixed_noise']
    out = []
    for q, rec in enumerate(g.models):
        ev = gp_state_oracle(P0, Y[:, q], rec.raw, 'matern52', flags, w, V[:, q], dtype=LD)
        out.append((ev,) + append_bars(ev, len(P0)))
    return out


# ------------------------------------------------------------------------------------------------ tests: update(append=True)
@pytest.mark.parametrize('kernel', [None, GK])
def test_three_appends_equal_one_fixed_noise_update(kernel):
    flags = 0 if kernel is None else kernel.flags
    g, eng = trained(kernel)
    h, _ = trained(kernel)
    P, A, S = measurements(g, 74)
    n0 = len(eng.calls)
    for a, b in ((0, 1), (1, 4), (4, 74)):
        g.update(P[a:b], A[a:b], S[a:b], append=True)
    assert names(eng, n0) == ['gp_state', 'gp_append', 'gp_append', 'gp_append', 'gp_append']       # the state once; 70 = 64 + 6
    assert [c[3:] for c in eng.calls[n0:] if c[0] == 'gp_append'] == [(13, 1), (16, 3), (80, 64), (86, 6)]
    assert [s['rows'] for s in g.append_info_] == [64, 6] and all(np.all(s['status'] == 0) for s in g.append_info_)
    h.update(P, A, S, fixed_noise=True)
    info, ref = g.gpr_info_, h.gpr_info_
    assert info['n_train'] == ref['n_train'] == 86 and info['n_added'] == 74 and g.Vr_sigma.shape == (86, 3) and np.all(g.Vr_sigma == 0)
    assert np.array_equal(info['noise_weight'], ref['noise_weight']) and np.array_equal(info['fixed_noise'], ref['fixed_noise'])
    assert np.array_equal(g._d['gp_P0'].numpy(), h._d['gp_P0'].numpy()) and np.array_equal(g._d['gp_Y'].numpy(), h._d['gp_Y'].numpy())
    assert g.P0.shape == (12, 2) and g.Vr.shape == (12, 3) and np.all(np.isnan(info['grad']))
    for q, (ev, rel, sc) in enumerate(held_bars(g, flags)):
        got = dict(Kinv=g._d['gp_Kinv'].numpy()[q], alpha=g._d['gp_alpha'].numpy()[q], logdet=g.append_info_[-1]['logdet'][q],
                   loss=info['loss'][q])
        for key, e in append_errors(got, ev).items():
            assert e <= rel * sc[key], (q, key, e, rel, sc[key])
        assert np.max(np.abs(got['Kinv'] - h._d['gp_Kinv'].numpy()[q])) <= 2 * rel * sc['Kinv']
        assert abs(info['loss'][q] - ref['loss'][q]) <= 2 * rel * sc['loss'] and g.models[q].loss == info['loss'][q]
    a, b = g.predict(P_STAR), h.predict(P_STAR)
    assert np.allclose(a[0], b[0], rtol=1e-9, atol=1e-12) and np.allclose(a[1], b[1], rtol=1e-9)


def test_append_false_makes_the_engine_calls_of_before():
    g, eng = trained()
    P, A, S = measurements(g, 3)
    n0 = len(eng.calls)
    g.update(P, A)
    g.update(P, A, S)
    g.update(P, A, S, fixed_noise=True)
    g.update(P, A, S, retrain=True)
    g.update(P, A, S, append=False)
    assert eng.calls[n0:] == [('gp_train', 'matern52', 0), ('gp_train', 'matern52', 0), ('gp_train_noise', 'matern52', 0, 0),
                              ('gp_train_noise', 'matern52', 0, 20), ('gp_train', 'matern52', 0)]
    assert g.gpr_info_['n_train'] == 15 and 'n_added' not in g.gpr_info_ and not hasattr(g, 'append_info_')
    k, eng2 = trained(GK)
    n0 = len(eng2.calls)
    k.update(P, A)
    k.update(P, A, S, fixed_noise=True)
    assert eng2.calls[n0:] == [('gp_train_ard', 'matern52', 3, 0), ('gp_train_noise', 'matern52', 3, 0)]


def test_append_after_a_plain_update_adds_to_its_points():
    g, eng = trained()
    P, A, S = measurements(g, 5)
    g.update(P[:3], A[:3])                                         # 15 points, all with the learned noise
    n0 = len(eng.calls)
    g.update(P[3:], A[3:], append=True)                            # no deviations: the learned noise again
    assert names(eng, n0) == ['gp_state', 'gp_append'] and g.gpr_info_['n_train'] == 17 and g.gpr_info_['n_added'] == 5
    assert np.array_equal(g.gpr_info_['noise_weight'], np.ones(17)) and np.all(g.gpr_info_['fixed_noise'] == 0)
    h, _ = trained()
    h.update(P, A)
    assert np.allclose(g._d['gp_Kinv'].numpy(), h._d['gp_Kinv'].numpy(), rtol=1e-8, atol=1e-8 * np.abs(h._d['gp_Kinv'].numpy()).max())
    g.update(P[:1], A[:1], S[:1], append=True)                     # the state is the object's own now: no further gp_state
    assert names(eng, n0) == ['gp_state', 'gp_append', 'gp_append'] and g.gpr_info_['n_train'] == 18
    assert np.array_equal(g.gpr_info_['noise_weight'], [1.0] * 17 + [0.0])
    g.update(P[:2], A[:2])                                         # a plain update replaces, as before, and drops the state
    assert g.gpr_info_['n_train'] == 14 and 'noise_weight' not in g.gpr_info_
    g.update(P[:1], A[:1], append=True)
    assert names(eng, n0)[-2:] == ['gp_state', 'gp_append'] and g.gpr_info_['n_train'] == 15


def test_retrain_with_append_trains_on_the_accumulated_noise_and_drops_the_state():
    g, eng = trained(max_iter=5)
    P, A, S = measurements(g, 6)
    g.update(P[:2], A[:2], S[:2], append=True)
    g.update(P[2:4], A[2:4], append=True)
    n0 = len(eng.calls)
    old = list(g.models)
    g.update(P[4:], A[4:], S[4:], retrain=True, append=True)
    assert eng.calls[n0:] == [('gp_train_noise', 'matern52', 0, 5)]
    V = np.zeros((18, 3))
    V[12:14], V[16:18] = (S[:2] / g.Sigma_r) ** 2, (S[4:] / g.Sigma_r) ** 2
    assert np.array_equal(g.gpr_info_['noise_weight'], [1.0] * 12 + [0.0] * 2 + [1.0] * 2 + [0.0] * 2)
    assert np.array_equal(g.gpr_info_['fixed_noise'], V) and g.gpr_info_['n_train'] == 18 and g.gpr_info_['n_added'] == 6
    assert all(a is not b for a, b in zip(g.models, old)) and np.array_equal(g.gpr_info_['iterations'], [5, 5, 5])
    g.update(P[:1], A[:1], S[:1], append=True)
    assert names(eng, n0) == ['gp_train_noise', 'gp_state', 'gp_append'] and g.gpr_info_['n_train'] == 19


def test_forget_keeps_the_simulations_and_the_last_points():
    g, eng = trained()
    P, A, S = measurements(g, 9)
    g.update(P[:5], A[:5], S[:5], append=True)
    g.update(P[5:], A[5:], append=True)
    before = g._d['gp_P0'].numpy().copy(), g.gpr_info_['fixed_noise'].copy()
    n0 = len(eng.calls)
    g.forget(keep_last=6)
    assert names(eng, n0) == ['gp_state'] and g.gpr_info_['n_train'] == 18 and g.gpr_info_['n_added'] == 6
    assert np.array_equal(g._d['gp_P0'].numpy(), np.concatenate([before[0][:12], before[0][15:]]))
    assert np.array_equal(g.gpr_info_['fixed_noise'], np.concatenate([before[1][:12], before[1][15:]]))
    assert np.array_equal(g.gpr_info_['noise_weight'], [1.0] * 12 + [0.0] * 2 + [1.0] * 4) and g.Vr_sigma.shape == (18, 3)
    g.update(P[:1], A[:1], S[:1], append=True)                     # forget left a state: the append needs no gp_state
    assert names(eng, n0) == ['gp_state', 'gp_append'] and g.gpr_info_['n_train'] == 19
    g.forget(keep_last=100)                                        # more than there are: every added point stays
    assert g.gpr_info_['n_train'] == 19
    g.forget()
    assert g.gpr_info_['n_train'] == 12 and g.gpr_info_['n_added'] == 0 and np.array_equal(g._d['gp_P0'].numpy(), g.P0)
    h, _ = trained()
    assert np.allclose(g.predict(P_STAR)[0], h.predict(P_STAR)[0], rtol=1e-9) and np.allclose(g.predict(P_STAR)[1], h.predict(P_STAR)[1], rtol=1e-9)
    with pytest.raises(ValueError, match='keep_last'):
        g.forget(keep_last=-1)


def test_the_limit_of_800_points():
    g, eng = trained(max_iter=3)
    P, A, S = measurements(g, 790, scale=0.2)
    g.update(P[:787], A[:787], S[:787], append=True)
    assert g.gpr_info_['n_train'] == 799 and [s['rows'] for s in g.append_info_] == [64] * 12 + [19]
    n = eng.launches
    with pytest.raises(NotImplementedError, match='forget'):
        g.update(P[787:789], A[787:789], S[787:789], append=True)   # 799 + 2
    assert eng.launches == n and g.gpr_info_['n_train'] == 799
    g.update(P[787:788], A[787:788], S[787:788], append=True)       # 799 + 1
    assert g.gpr_info_['n_train'] == 800 and eng.launches == n + 1
    with pytest.raises(NotImplementedError, match='forget'):
        g.update(P[788:789], A[788:789], S[788:789], append=True)
    g.forget(keep_last=10)
    g.update(P[788:789], A[788:789], S[788:789], append=True)
    assert g.gpr_info_['n_train'] == 23


def test_refusals_come_before_any_engine_call():
    g, eng = trained(max_iter=3)
    P, A, S = measurements(g, 3)
    state = (g._d['gp_Kinv'], g.gpr_info_['n_train'], g.Vr_sigma.copy(), list(g.models))
    eng.launches = 0
    with pytest.raises(NotImplementedError, match='retrain=True.*A_sigma_new'):
        g.update(P, A, retrain=True, append=True)
    bad, nan, inf = S.copy(), S.copy(), S.copy()
    bad[1, 2], nan[0, 0], inf[2, 1] = -1e-3, np.nan, np.inf
    for kw in (dict(), dict(retrain=True)):
        for sig, text in ((bad, 'finite and >= 0'), (nan, 'finite and >= 0'), (inf, 'finite and >= 0'), (S[:2], 'must have shape'),
                          (S[:, :2], 'must have shape'), (S[0], 'must have shape')):
            with pytest.raises(ValueError, match=text):
                g.update(P, A, sig, append=True, **kw)
        with pytest.raises(ValueError, match='A_new must have shape'):
            g.update(P, A[:2], S, append=True, **kw)
        with pytest.raises(ValueError, match='must be finite'):
            g.update(P, np.where(np.arange(3)[:, None] == 1, np.nan, A), S, append=True, **kw)
        with pytest.raises(ValueError, match='must be finite'):
            g.update(np.array([[1.0, np.inf]]), A[:1], S[:1], append=True, **kw)
        with pytest.raises(ValueError, match='must have shape'):
            g.update(np.ones((3, 5)), A, S, append=True, **kw)
        with pytest.raises(NotImplementedError, match='forget'):
            g.update(np.ones((800, 2)), np.ones((800, 3)), np.ones((800, 3)), append=True, **kw)
    assert eng.launches == 0
    assert g._d['gp_Kinv'] is state[0] and g.gpr_info_['n_train'] == state[1] and np.array_equal(g.Vr_sigma, state[2])
    assert g.models == state[3] and 'noise_weight' not in g.gpr_info_ and not hasattr(g, 'append_info_')
    fresh = fitted2(GpAppendNumpyEngine())
    with pytest.raises(AttributeError, match="no attribute 'models'"):
        fresh.update(P, A, S, append=True)
    with pytest.raises(AttributeError, match="no attribute 'models'"):
        fresh.forget()


@pytest.mark.parametrize('kernel', [None, GK])
def test_engine_without_the_append_calls_is_refused(kernel):
    eng = GpNoiseNumpyEngine()
    g, _ = trained(kernel, max_iter=2, eng=eng)
    P, A, S = measurements(g, 3)
    n = eng.launches
    with pytest.raises(NotImplementedError, match="no 'gp_state' .*no CPU fallback"):
        g.update(P, A, S, append=True)
    with pytest.raises(NotImplementedError, match="no 'gp_state' .*no CPU fallback"):
        g.forget()
    assert eng.launches == n
    g.update(P, A, S, fixed_noise=True)                            # the updates of before ask for their own calls only
    assert g.gpr_info_['n_train'] == 15


def test_the_previous_state_survives_a_failed_pivot():
    g, eng = trained()
    P, A, S = measurements(g, 4)
    g.update(P[:2], A[:2], S[:2], append=True)
    kept = (g._d['gp_Kinv'], g._d['gp_alpha'], g._d['gp_P0'], g._gp_X, g.gpr_info_['n_train'], g.gpr_info_['loss'].copy(),
            g.append_info_, g.predict(P_STAR))
    eng.fail_modes = (1,)
    with pytest.raises(np.linalg.LinAlgError, match=r'mode\(s\) \[2\].*status \[1\]'):
        g.update(P[2:], A[2:], S[2:], append=True)
    assert g._d['gp_Kinv'] is kept[0] and g._d['gp_alpha'] is kept[1] and g._d['gp_P0'] is kept[2] and g._gp_X is kept[3]
    assert g.gpr_info_['n_train'] == kept[4] == 14 and np.array_equal(g.gpr_info_['loss'], kept[5]) and g.append_info_ is kept[6]
    again = g.predict(P_STAR)
    assert np.array_equal(again[0], kept[7][0]) and np.array_equal(again[1], kept[7][1])
    n0 = len(eng.calls)
    g.update(P[2:], A[2:], S[2:], append=True)                     # and the same call goes through from that state
    assert names(eng, n0) == ['gp_append'] and g.gpr_info_['n_train'] == 16
    # an exact copy of an exact point: S is a few eps C of either sign, below m' eps C in every mode
    g.update(P[:1], A[:1], np.zeros((1, 3)), append=True)
    with pytest.raises(np.linalg.LinAlgError, match=r'mode\(s\) \[1, 2, 3\].*status \[1, 1, 1\]'):
        g.update(P[:1], A[:1] + 1.0, np.zeros((1, 3)), append=True)
    assert g.gpr_info_['n_train'] == 17 and np.all(np.isfinite(g.predict(P_STAR)[0]))


def test_pickle_round_trip_then_append():
    g, eng = trained(GK)
    P, A, S = measurements(g, 5)
    g.update(P[:3], A[:3], S[:3], append=True)
    blob = pickle.dumps(g)
    assert not any(k.startswith('_gp_') for k in g.__getstate__())                     # X and logdet stay behind
    h = pickle.loads(blob)
    assert set(h._d.stash) >= {'gp_P0', 'gp_Y', 'gp_raw', 'gp_Kinv', 'gp_alpha'} and h._d.stash['gp_P0'].shape == (15, 2)
    assert np.array_equal(h.gpr_info_['noise_weight'], g.gpr_info_['noise_weight']) and h.gpr_info_['n_added'] == 3
    assert np.array_equal(h.gpr_info_['fixed_noise'], g.gpr_info_['fixed_noise'])
    h._eng = eng2 = GpAppendNumpyEngine()
    want = g.predict(P_STAR)
    got = h.predict(P_STAR)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    h.update(P[3:], A[3:], S[3:], append=True)
    g.update(P[3:], A[3:], S[3:], append=True)
    assert names(eng2) == ['gp_state', 'gp_append'] and h.gpr_info_['n_train'] == 17
    assert np.allclose(h._d['gp_Kinv'].numpy(), g._d['gp_Kinv'].numpy(), rtol=1e-9, atol=1e-9 * np.abs(g._d['gp_Kinv'].numpy()).max())
    assert np.allclose(h.predict(P_STAR)[0], g.predict(P_STAR)[0], rtol=1e-9)


# ------------------------------------------------------------------------------------------------ tests: the C entry points
INVALID, UNSUPPORTED = -1, -2
PTR = [8 * (i + 1) for i in range(16)]
STATE_NAMES = 'P0 m d ldp Y r ldy w V ldv kernel flags raw Kinv alpha info X logdet ws ws_bytes stream'
APPEND_NAMES = 'P0 m d ldp Y r ldy w V ldv k kernel flags raw X Kinv logdet X2 Kinv2 alpha2 logdet2 info ws ws_bytes stream'
GOOD = dict(P0=PTR[0], m=10, d=2, ldp=2, Y=PTR[1], r=3, ldy=3, w=PTR[2], V=PTR[3], ldv=3, k=4, kernel=0, flags=3, raw=PTR[4], X=PTR[5],
            Kinv=PTR[6], logdet=PTR[7], X2=PTR[8], Kinv2=PTR[9], alpha2=PTR[10], logdet2=PTR[11], info=PTR[12], alpha=PTR[13], ws=PTR[14],
            ws_bytes=1 << 40, stream=None)
ENTRY_CASES = [
    ('spr_gp_append_f64', {'X': None}, INVALID, 'NULL'), ('spr_gp_append_f64', {'logdet2': None}, INVALID, 'NULL'),
    ('spr_gp_append_f64', {'w': None}, INVALID, 'NULL'), ('spr_gp_append_f64', {'ldy': 2}, INVALID, 'bad shape'),
    ('spr_gp_append_f64', {'ldv': 2}, INVALID, 'bad shape r=3 ldv=2'), ('spr_gp_append_f64', {'k': 0}, INVALID, 'k = 0 new rows'),
    ('spr_gp_append_f64', {'k': 10}, INVALID, 'k = 10 new rows of m = 10'), ('spr_gp_append_f64', {'kernel': 4}, INVALID, 'kernel code'),
    ('spr_gp_append_f64', {'flags': 4}, INVALID, 'flags'), ('spr_gp_append_f64', {'m': 100, 'k': 65}, UNSUPPORTED, 'k = 65 new rows exceed 64'),
    ('spr_gp_append_f64', {'m': 801}, UNSUPPORTED, 'm = 801 exceeds 800'),
    ('spr_gp_append_f64', {'d': 9, 'ldp': 9, 'flags': 1}, UNSUPPORTED, 'exceeds 8'),
    ('spr_gp_append_f64', {'ws_bytes': 'one short'}, INVALID, 'workspace of'), ('spr_gp_append_f64', {'ws': 12}, INVALID, '8-byte aligned'),
    ('spr_gp_state_f64', {'X': None}, INVALID, 'NULL'), ('spr_gp_state_f64', {'logdet': None}, INVALID, 'NULL'),
    ('spr_gp_state_f64', {'m': 0}, INVALID, 'bad shape'), ('spr_gp_state_f64', {'ldv': 2}, INVALID, 'bad shape r=3 ldv=2'),
    ('spr_gp_state_f64', {'flags': -1}, INVALID, 'flags'), ('spr_gp_state_f64', {'m': 801}, UNSUPPORTED, 'exceeds 800'),
    ('spr_gp_state_f64', {'ws_bytes': 'one short'}, INVALID, 'workspace of'),
]


@pytest.mark.parametrize('case', ENTRY_CASES, ids=lambda c: c[0][7:-4] + ':' + '+'.join(f'{k}={v}' for k, v in c[1].items()))
def test_entry_point_refusal(case):
    from openmeasure_amd import _lib
    fn, change, status, fragment = case
    lib = _lib.load()
    args = dict(GOOD, **change)
    if args['ws_bytes'] == 'one short':
        if fn == 'spr_gp_append_f64':
            need = lib.spr_gp_workspace_append(args['m'], args['d'], args['k'], args['r'])
            assert need == 8 * args['r'] * args['m'] * (args['d'] + 2 * args['k'])
        else:
            need = lib.spr_gp_workspace_ard(args['m'], args['d'], args['r'])
        args['ws_bytes'] = need - 1
    rc = getattr(lib, fn)(*[args[n] for n in (APPEND_NAMES if fn == 'spr_gp_append_f64' else STATE_NAMES).split()])
    text = lib.spr_last_error().decode()
    assert rc == status, (rc, text)
    assert text.startswith(fn + ': ') and fragment in text, text


def test_append_workspace_of_refused_shapes_is_zero():
    from openmeasure_amd import _lib
    lib = _lib.load()
    assert _lib.SPR_GP_MAX_APPEND == 64
    assert lib.spr_gp_workspace_append(800, 3, 64, 2) == 8 * 2 * 800 * (3 + 128)
    for m, d, k, r in ((801, 3, 1, 1), (10, 3, 0, 1), (10, 3, 65, 1), (10, 3, 10, 1), (10, 0, 1, 1), (10, 3, 1, 0)):
        assert lib.spr_gp_workspace_append(m, d, k, r) == 0
