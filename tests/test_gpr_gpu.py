"""csrc/gp.hip on the GPU against the NumPy oracle of tests/test_gpr_host.py, at the smallest shapes where the kernels can go
wrong.  The kernel's edges are the block row of 16, the LDS chunk of 32 contraction rows and the 256 threads that each own
one column: m in {1, 2, 37, 64, 65, 130} (one row; inside a block; at and one past a multiple of 16 and 32; several blocks
and chunks with a tail) and m in {256, 257, 530} (one full group of columns; one column in a second group; three groups
with a tail -- the passes over column groups and their panel starts), d in {1, 3}, r in {1, 5}, all four kernels, Y with a
row stride.

THE BAR of the factor-only tests (stated before the first GPU run).  rel = c m eps kappa_2(K), eps = 2^-53, c = 16:
* 12 = 3 x 4.  Higham, Accuracy and Stability, Thm 10.4: the Cholesky solve has the backward error |dK| <= gamma_{3m+1}
  |R^T| |R|, normwise about 3 m eps |K| for matrices like these whose |R^T||R| is of the size of K.  The kernel forms four
  things explicitly -- the factor, the inverse of the factor, the product X^T X, the product K^-1 res -- each with a backward
  error of that form: 4 x 3.
* 4 more for forming K: every entry carries a few eps from the division by l, the polynomial and exp / log1p of the device
  library (<= 2 ulp) in l and in the entry, an absolute perturbation of <= 4 eps per entry, |dK|_2 <= 4 m eps <= 4 m eps |K|_2.
A backward error of rel / kappa in K moves K^-1 by rel |K^-1|_2 and alpha by rel |K^-1|_2 |res|_2, so each quantity is held
to rel times a norm bound on its sum of absolute terms (scales() below): K^-1 to sK = |K^-1|_2, alpha to sa = sK |res|_2,
the loss to (sa |res| / 2 + sum |log r_jj^2| / 2 + m log(2 pi) / 2) / m, the gradients to sigmoid(raw_l) (sK + sa^2) sum|l dK/dl|
/ (2 m l), sigmoid(raw_n) (m sK + sa^2) / 2m and sa / sqrt(m).  The reference values are the oracle in np.longdouble, kappa is
taken from its K.  Inputs are chosen so that rel < 1e-8 (asserted): the near-floor case (noise 2.2e-4) uses l = 0.049.

Trajectory bar: Adam's step is lr m^ / (sqrt(v^) + 1e-8); a gradient error dg_c changes it by at most 2 lr dg_c / sqrt(v^_c)
(numerator and denominator).  With dg_c = rel x the gradient's scale above at evaluation i, the bar of parameter c at
evaluation j is  sum_{i < j} 2 x 2 lr max_{i' <= i} dg_c / sqrt(v^_c,i) + 8 eps (|p_c| + lr) j  -- the second factor 2 for the
differences already made, which later gradients see (the map does not expand them: trajectories move by 1e-12 under a 1e-12
perturbation), the last term for the roundings of the update itself."""
import numpy as np
import pytest

from tests.test_gpr_host import (KERNELS, GpNumpyEngine, field_case, gp_case, gp_distance, gp_kernel, gp_loss_grad, gp_predict,
                                 gp_train, sigmoid, softplus)

pytestmark = pytest.mark.gpu
LD = np.longdouble
EPS = 2.0 ** -53
C_BAR = 16
RAWS = [(0.0, 0.0, 0.0), (-3.0, -9.0, 0.03), (0.8, -3.0, -0.01)]      # the start; noise near its floor; a long lengthscale
LOG_2PI = np.log(2.0 * np.pi)


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


def scales(ev, raw, m):
    """norm bounds on the sums of absolute terms (module docstring), from an oracle evaluation"""
    f = lambda a: np.asarray(a, dtype=np.float64)
    sK = np.linalg.norm(f(ev['Kinv']), 2)
    rn = np.linalg.norm(f(ev['res']))
    sa = sK * rn
    ell = float(softplus(np.float64(raw[0])))
    return dict(Kinv=sK, alpha=sa, loss=(0.5 * sa * rn + 0.5 * np.sum(np.abs(f(ev['logdiag']))) + 0.5 * m * LOG_2PI) / m,
                grad=np.array([float(sigmoid(np.float64(raw[0]))) * (sK + sa * sa) * np.sum(np.abs(f(ev['dk']))) / (2 * m * ell),
                               float(sigmoid(np.float64(raw[1]))) * (m * sK + sa * sa) / (2 * m), sa / np.sqrt(m)]))


def rel_bar(ev, m):
    rel = C_BAR * m * EPS * np.linalg.cond(np.asarray(ev['K'], dtype=np.float64))
    assert rel < 1e-8, rel
    return rel


@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('m,d,r', [(1, 1, 1), (1, 3, 5), (2, 1, 5), (2, 3, 1), (37, 1, 1), (37, 3, 5), (64, 1, 5), (64, 3, 1),
                                   (65, 1, 1), (65, 3, 5), (130, 1, 5), (130, 3, 1), (256, 3, 1), (257, 3, 5), (530, 3, 1)])
def test_factor_only(eng, m, d, r, kernel):
    """max_iter = 0 at fixed raw (mode q takes RAWS[q % 3]; with r = 1, RAWS[(m + d) % 3]): alpha, K^-1, loss and gradient
    against the longdouble oracle at the bar of the module docstring."""
    P0, Y = gp_case(m, d, r, seed=m + d)
    raws = np.array([RAWS[(q if r > 1 else m + d) % 3] for q in range(r)])
    raw, Kinv, alpha, info, tr = eng.gp_train(eng.to_device(P0), strided(eng, Y), kernel, eng.to_device(raws), 0.1, 0, 0.0)
    raw, Kinv, alpha, info = (eng.to_host(t) for t in (raw, Kinv, alpha, info))
    assert tr is None and np.array_equal(raw, raws) and np.all(info[:, 0] == 0) and np.all(info[:, 3] == 0)
    D = gp_distance(P0.astype(LD))
    for q in range(r):
        ev = gp_loss_grad(D, Y[:, q], raws[q], kernel, dtype=LD)
        rel, sc = rel_bar(ev, m), scales(ev, raws[q], m)
        errs = dict(Kinv=np.max(np.abs(Kinv[q] - ev['Kinv'])) / sc['Kinv'], alpha=np.max(np.abs(alpha[q] - ev['alpha'])) / sc['alpha'],
                    loss=abs(info[q, 1] - ev['loss']) / sc['loss'], grad=np.max(np.abs(info[q, 4:7] - ev['grad']) / sc['grad']))
        print(f'factor m={m} d={d} {kernel} mode {q} raw={raws[q].tolist()}: bar {rel:.2e} errors ' +
              ' '.join(f'{k} {float(v):.2e}' for k, v in errs.items()))
        assert np.array_equal(Kinv[q], Kinv[q].T)                # both halves add the same products in the same order
        for k, v in errs.items():
            assert v <= rel, (k, float(v), rel)


@pytest.mark.parametrize('m,d,kernel', [(37, 1, 'matern52'), (64, 1, 'matern12'), (65, 3, 'rbf'), (130, 3, 'matern32')])
def test_trajectory_of_25_evaluations(eng, m, d, kernel):
    """The trace of 25 evaluations (rel_error = 0), parameter by parameter, against the float64 oracle at the trajectory bar
    of the module docstring."""
    r, n_it, lr = 3, 25, 0.1
    P0, Y = gp_case(m, d, r, seed=10 + m, noise=0.3)
    raw, Kinv, alpha, info, tr = eng.gp_train(eng.to_device(P0), strided(eng, Y), kernel, eng.zeros((r, 3)), lr, n_it, 0.0,
                                              trace=True)
    tr, info, raw = eng.to_host(tr), eng.to_host(info), eng.to_host(raw)
    assert np.all(info[:, 0] == n_it) and np.all(info[:, 3] == 0)
    D = gp_distance(P0)
    for q in range(r):
        t = gp_train(D, Y[:, q], kernel, lr=lr, max_iter=n_it, tol=0.0)
        bar, dg_max, v, b2t, worst = np.zeros(3), np.zeros(3), np.zeros(3), 1.0, 0.0
        for j in range(n_it):
            p = t['trace'][j, 1:]
            ev = gp_loss_grad(D, Y[:, q], p, kernel)
            rel, sc = rel_bar(ev, m), scales(ev, p, m)
            dp = np.abs(tr[q, j, 1:] - p)
            dl = abs(tr[q, j, 0] - t['trace'][j, 0])
            bar_j = bar + 8 * EPS * (np.abs(p) + lr) * j
            worst = max(worst, float(np.max(dp / np.maximum(bar_j, 1e-300))) if j else 0.0)
            assert np.all(dp <= bar_j), (q, j, dp, bar_j)
            assert dl <= rel * sc['loss'] + np.sum(np.abs(ev['grad']) * bar_j), (q, j, dl)
            dg_max = np.maximum(dg_max, rel * sc['grad'])
            b2t *= 0.999
            v = 0.999 * v + 0.001 * ev['grad'] ** 2
            bar = bar + 2 * 2 * lr * dg_max / np.sqrt(v / (1 - b2t))
        print(f'trajectory m={m} d={d} {kernel} mode {q}: max |d raw| {np.max(np.abs(tr[q, :, 1:] - t["trace"][:, 1:])):.2e} '
              f'final bar {bar.tolist()} worst ratio {worst:.2e}')
        assert np.all(np.abs(raw[q] - t['raw']) <= bar + 8 * EPS * (np.abs(t['raw']) + lr) * n_it)


@pytest.mark.parametrize('m,d,seed,bar', [(37, 1, 5, 7.3e-12), (130, 3, 4, 1.5e-11)])
def test_training_to_convergence(eng, m, d, seed, bar):
    """Default training (max_iter 1000, rel_error 1e-5, lr 0.1, Matern-5/2) of 5 modes on gp_case(m, d, 5, seed, noise=0.3).
    The oracle stops after 108/104/104/90/106 (m = 37) and 107/102/92/216/189 (m = 130) evaluations, and its last two e lie
    more than 1 % away from rel_error in every mode (checked on the CPU, asserted again here), so the evaluation count must be
    equal.  The bar on the final raw is MEASURED: ten times the larger of the final differences between the float64 oracle
    and (a) the float64 oracle with K^-1 and log det from LU (route='inv'), (b) the longdouble oracle, over the five modes --
    m = 37: (a) 7.21e-13, (b) 5.92e-13 -> 7.3e-12;  m = 130: (a) 1.42e-12, (b) 1.31e-12 -> 1.5e-11."""
    r, tol = 5, 1e-5
    P0, Y = gp_case(m, d, r, seed=seed, noise=0.3)
    raw, Kinv, alpha, info, _ = eng.gp_train(eng.to_device(P0), strided(eng, Y), 'matern52', eng.zeros((r, 3)), 0.1, 1000, tol)
    raw, info = eng.to_host(raw), eng.to_host(info)
    D = gp_distance(P0)
    for q in range(r):
        t = gp_train(D, Y[:, q], 'matern52')
        es = np.abs(np.diff(t['trace'][:, 0]))
        assert abs(t['e'] / tol - 1) > 0.01 and abs(es[-2] / tol - 1) > 0.01 and t['iterations'] < 1000
        print(f'training m={m} mode {q}: evaluations {int(info[q, 0])} / {t["iterations"]}, e {info[q, 2]:.3e} / {float(t["e"]):.3e}, '
              f'max |d raw| {np.max(np.abs(raw[q] - t["raw"])):.2e} (bar {bar:.1e})')
    for q in range(r):
        t = gp_train(D, Y[:, q], 'matern52')
        assert info[q, 3] == 0 and int(info[q, 0]) == t['iterations']
        assert np.max(np.abs(raw[q] - t['raw'])) <= bar


@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('m,d,n_p', [(37, 1, 1), (65, 3, 70), (130, 3, 70), (2, 1, 70), (300, 3, 70)])
def test_predict_against_the_closed_form(eng, m, d, n_p, kernel):
    """mean = mu + k*.alpha, var = max(1 - k*^T K^-1 k*, 0) + s2 against longdouble at rel = c m eps kappa times the sums of
    absolute terms (|mu| + |k*|_2 sa;  1 + |k*|_2^2 sK + s2).  Row 0 of P_star is a training point; with n_p = 70, row 1 lies
    1000 units away: every kernel underflows to 0 there, the mean is mu and the variance 1 + s2 to rounding."""
    r = 5
    P0, Y = gp_case(m, d, r, seed=20 + m)
    raws = np.array([RAWS[q % 3] for q in range(r)])
    rng = np.random.default_rng(m)
    Ps = rng.standard_normal((n_p, d)) * 1.5
    Ps[0] = P0[min(3, m - 1)]
    if n_p > 1:
        Ps[1] = P0.mean(axis=0) + 1000.0
    P0_d = eng.to_device(P0)
    raw, Kinv, alpha, info, _ = eng.gp_train(P0_d, eng.to_device(Y), kernel, eng.to_device(raws), 0.1, 0, 0.0)
    mean, var = eng.gp_predict(P0_d, eng.to_device(Ps), kernel, raw, Kinv, alpha)
    mean, var = eng.to_host(mean), eng.to_host(var)
    assert mean.shape == var.shape == (n_p, r)
    D = gp_distance(P0.astype(LD))
    evs = [gp_loss_grad(D, Y[:, q], raws[q], kernel, dtype=LD) for q in range(r)]
    want_m, want_v = gp_predict(P0.astype(LD), Ps.astype(LD), raws.astype(LD), np.stack([e['Kinv'] for e in evs]),
                                np.stack([e['alpha'] for e in evs]), kernel)
    Ds = gp_distance(Ps, P0)
    worst = 0.0
    for q in range(r):
        rel, sc = rel_bar(evs[q], m), scales(evs[q], raws[q], m)
        s2 = float(softplus(raws[q, 1])) + 1e-4
        kn = np.linalg.norm(gp_kernel(kernel, Ds / float(softplus(raws[q, 0])))[0], axis=1)
        em = np.abs(mean[:, q] - want_m[:, q]) / (abs(raws[q, 2]) + kn * sc['alpha'] + 1e-300)
        evr = np.abs(var[:, q] - want_v[:, q]) / (1 + kn * kn * sc['Kinv'] + s2)
        worst = max(worst, float(np.max(em)) / rel, float(np.max(evr)) / rel)
        assert np.all(em <= rel) and np.all(evr <= rel), (q, float(np.max(em)), float(np.max(evr)), rel)
        assert np.all(var[:, q] >= s2 * (1 - 4 * EPS))
        if n_p > 1:
            assert abs(var[1, q] - (1 + s2)) <= 4 * EPS * (1 + s2) and abs(mean[1, q] - raws[q, 2]) <= EPS * abs(raws[q, 2])
    print(f'predict m={m} d={d} n_p={n_p} {kernel}: worst error / bar {worst:.2e}')


def test_end_to_end_against_the_oracle_driven_double(eng):
    """The public GPR on the HIP engine against the same class over the oracle-driven engine double of the host test, after
    60 evaluations (rel_error = 0: no stopping decision).  The two sets of hyper-parameters agree to the 1e-11 of the
    training test; coefficients and fields are smooth in them with a sensitivity of at most kappa(K), so every output is held
    to 1e-11 kappa_max (kappa from the oracle's K at the trained values) relative to its largest entry."""
    from openmeasure_amd.gpr import GPR
    X, F, P = field_case()
    out = []
    for e in (eng, GpNumpyEngine()):
        g = GPR(X, F, None, P, engine=e)
        g.fit(select_modes='number', n_modes=3)
        g.train(max_iter=60, rel_error=0.0)
        P_star = np.array([[2.2, 320.0], [3.3, 341.0], P[4]])
        A_pred, A_sigma = g.predict(P_star)
        out.append((g, A_pred, A_sigma, g.reconstruct(A_pred), g.reconstruct_std(A_sigma)))
    (g, *dev), (h, *ref) = out
    assert np.array_equal(g.gpr_info_['iterations'], [60, 60, 60]) and np.array_equal(h.gpr_info_['iterations'], [60, 60, 60])
    sign = np.sign(np.sum(g.Vr * h.Vr, axis=0))                # a POD mode's sign is arbitrary between two eigensolvers
    D = gp_distance(h.P0)
    kappa = max(np.linalg.cond(gp_loss_grad(D, h.Vr[:, i], q.raw, 'matern52')['K']) for i, q in enumerate(h.models))
    tol = 1e-11 * kappa
    names = ('A_pred', 'A_sigma', 'field', 'field std')
    dev[0] = dev[0] * sign
    for name, a, b in zip(names, dev, ref):
        err = np.max(np.abs(a - b)) / np.max(np.abs(b))
        print(f'end to end {name}: relative error {err:.2e} (bar {tol:.2e}, kappa {kappa:.2e})')
    for name, a, b in zip(names, dev, ref):
        assert a.shape == b.shape and np.max(np.abs(a - b)) <= tol * np.max(np.abs(b)), name
    # the device tensors of predict(to_host=False) go straight into reconstruct / reconstruct_std
    Ad, Sd = g.predict(np.array([[2.2, 320.0], [3.3, 341.0], P[4]]), to_host=False)
    assert Ad.is_cuda and np.array_equal(g.reconstruct(Ad), dev[2]) and np.array_equal(g.reconstruct_std(Sd), dev[3])


def test_two_runs_agree_bit_for_bit(eng):
    m, d, r = 130, 3, 5
    P0, Y = gp_case(m, d, r, seed=7, noise=0.3)
    Ps = np.random.default_rng(1).standard_normal((70, d))
    runs = []
    for _ in range(2):
        P0_d = eng.to_device(P0)
        raw, Kinv, alpha, info, tr = eng.gp_train(P0_d, strided(eng, Y), 'matern52', eng.zeros((r, 3)), 0.1, 30, 1e-5, trace=True)
        mean, var = eng.gp_predict(P0_d, eng.to_device(Ps), 'matern52', raw, Kinv, alpha)
        runs.append([eng.to_host(t) for t in (raw, Kinv, alpha, info, tr, mean, var)])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def test_a_pivot_that_is_not_finite_stops_its_mode_only(eng):
    """raw_n = NaN in mode 0 makes its first pivot NaN: status 2 for that mode, raw left as given, no evaluation counted; mode 1
    trains as if alone."""
    P0, Y = gp_case(37, 1, 2, seed=3)
    raws = np.array([[0.0, np.nan, 0.0], [0.0, 0.0, 0.0]])
    raw, Kinv, alpha, info, _ = eng.gp_train(eng.to_device(P0), eng.to_device(Y), 'matern52', eng.to_device(raws), 0.1, 5, 0.0)
    info, raw = eng.to_host(info), eng.to_host(raw)
    assert info[0, 3] == 2 and info[0, 0] == 0 and np.array_equal(raw[0], raws[0], equal_nan=True)
    t = gp_train(gp_distance(P0), Y[:, 1], 'matern52', max_iter=5, tol=0.0)
    assert info[1, 3] == 0 and info[1, 0] == 5 and np.allclose(raw[1], t['raw'], rtol=0, atol=1e-12)
