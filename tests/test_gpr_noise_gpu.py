"""spr_gp_train_noise_f64 (csrc/gp.hip, engine.gp_train_noise) on the GPU against the NumPy oracle of
tests/test_gpr_noise_host.py, at the kernel's edges rather than the workload's (the rationale of tests/test_gpr_gpu.py): the block
row of 16, the LDS chunk of 32 contraction rows and the 256 threads that each own one column -- m in {1, 2, 37, 65, 130, 257} --
with (d, flags) in {(3, plain), (1, scale), (3, ARD), (3, both), (8, both)}, r in {1, 5}, Y AND V with a padded row stride.

The noise case of every test: the last k = max(1, m // 4) points carry a given variance, w = 0 and V = (0.15 + 0.3 u)^2 there
(noise_case of the host file, seed 1000 + m + d), the others the learned one (w = 1, V = 0).  At m = 1 no point carries s2: the
noise gradient must be exactly 0.

THE BARS are those of tests/test_gpr_ard_gpu.py (its module docstring): rel = (16 + d + |zmax|_2) m eps kappa_2(K) with K
including diag(n) -- forming the diagonal adds one fma to an entry that already has its (4 + d) eps -- times the scales of its
scales(), with one change: the noise gradient sigmoid(raw_n) sum_i w_i (K^-1_ii - alpha_i^2) / 2m has the sum of absolute terms
sigmoid(raw_n) (|w|_1 sK + max(w) sa^2) / 2m.  (d, flags) = (1, 0) is not among the cases: at m = 130 its inputs give rel = 3.8e-8,
above the cap rel < 1e-8 that rel_bar asserts, so the plain model runs at d = 3, where every case stays below it.  The trajectory bar is that file's, over these scales."""
import numpy as np
import pytest

from openmeasure_amd.gpr import GPR, GPKernel
from tests.test_gpr_ard_gpu import factor_inputs, rel_bar, scales, strided
from tests.test_gpr_ard_host import gp2_loss_grad, gp2_train, layout, split
from tests.test_gpr_host import KERNELS, field_case, gp_case, sigmoid, softplus
from tests.test_gpr_noise_host import GpNoiseNumpyEngine, gp2_loss_grad_noise, gp2_train_noise, noise_case

pytestmark = pytest.mark.gpu
LD = np.longdouble
EPS = 2.0 ** -53
F64 = lambda a: np.asarray(a, dtype=np.float64)


@pytest.fixture(scope='module')
def eng():
    from openmeasure_amd.engine import HipEngine
    return HipEngine('cuda:0')


def noise_scales(ev, raw, m, d, flags, w):
    """scales() of tests/test_gpr_ard_gpu.py with the weighted noise gradient's sum of absolute terms (module docstring)"""
    L, S, _ = layout(d, flags)
    sc = scales(ev, raw, m, d, flags)
    sK = sc['Kinv']
    sa = sc['alpha']
    sc['grad'][L + S] = float(sigmoid(np.float64(raw[L + S]))) * (np.sum(np.abs(w)) * sK + np.max(w) * sa * sa) / (2 * m)
    return sc


def device_noise(eng, w, V):
    return eng.to_device(w), strided(eng, V, pad=2)


FACTOR_M = [(1, 5), (2, 1), (37, 5), (65, 1), (130, 5), (257, 1)]                   # m and r, alternating
FACTOR_CASES = [(m, r, d, flags, kernel) for m, r in FACTOR_M for d, flags in ((3, 0), (1, 2), (3, 1), (3, 3), (8, 3))
                for kernel in (KERNELS if m == 37 else ('matern52',))]


@pytest.mark.parametrize('m,r,d,flags,kernel', FACTOR_CASES)
def test_factor_only(eng, m, r, d, flags, kernel):
    """max_iter = 0 at the raw settings of tests/test_gpr_ard_gpu.factor_inputs with the noise case of the module docstring:
    alpha, K^-1, loss and every gradient component against the longdouble oracle at the bar of the module docstring."""
    P0, Y, raws = factor_inputs(m, r, d, flags)
    w, V = noise_case(m, r, seed=1000 + m + d)
    n_par = layout(d, flags)[2]
    w_d, V_d = device_noise(eng, w, V)
    raw, Kinv, alpha, info, tr = eng.gp_train_noise(eng.to_device(P0), strided(eng, Y), w_d, V_d, kernel, flags, eng.to_device(raws),
                                                    0.1, 0, 0.0)
    raw, Kinv, alpha, info = (eng.to_host(t) for t in (raw, Kinv, alpha, info))
    assert tr is None and np.array_equal(raw, raws) and info.shape == (r, 4 + n_par)
    assert np.all(info[:, 0] == 0) and np.all(info[:, 3] == 0)
    for q in range(r):
        ev = gp2_loss_grad_noise(P0, Y[:, q], raws[q], kernel, flags, w, V[:, q], dtype=LD)
        rel, sc = rel_bar(ev, P0, m), noise_scales(ev, raws[q], m, d, flags, w)
        errs = dict(Kinv=np.max(np.abs(Kinv[q] - ev['Kinv'])), alpha=np.max(np.abs(alpha[q] - ev['alpha'])),
                    loss=abs(info[q, 1] - ev['loss']))
        errs.update({f'grad{c}': abs(info[q, 4 + c] - ev['grad'][c]) for c in range(n_par)})
        bars = dict(Kinv=sc['Kinv'], alpha=sc['alpha'], loss=sc['loss'], **{f'grad{c}': sc['grad'][c] for c in range(n_par)})
        print(f'factor m={m} d={d} flags={flags} {kernel} mode {q}: bar {rel:.2e} errors / scale ' +
              ' '.join(f'{k} {float(v) / max(bars[k], 1e-300):.2e}' for k, v in errs.items()))
        assert np.array_equal(Kinv[q], Kinv[q].T)                # both halves add the same products in the same order
        for k, v in errs.items():
            assert v <= rel * bars[k], (k, float(v), rel, bars[k])
        if m == 1:
            assert info[q, 4 + n_par - 2] == 0.0                 # no point carries s2


@pytest.mark.parametrize('flags', [0, 1, 2, 3])
@pytest.mark.parametrize('m', [37, 257])
def test_unit_weights_and_no_fixed_noise_are_the_existing_entry_point(eng, m, flags):
    """w = 1, V = 0: every operation multiplies by 1.0 or adds 0.0, so 25 evaluations with trace return the bits of
    gp_train_ard on the same inputs."""
    d, r, kernel, n_it = 3, 3, 'matern52', 25
    n_par = layout(d, flags)[2]
    P0, Y = gp_case(m, d, r, seed=40 + m, noise=0.3)
    P0_d = eng.to_device(P0)
    w_d, V_d = device_noise(eng, np.ones(m), np.zeros((m, r)))
    old = eng.gp_train_ard(P0_d, strided(eng, Y), kernel, flags, eng.zeros((r, n_par)), 0.1, n_it, 0.0, trace=True)
    new = eng.gp_train_noise(P0_d, strided(eng, Y), w_d, V_d, kernel, flags, eng.zeros((r, n_par)), 0.1, n_it, 0.0, trace=True)
    for name, a, b in zip(('raw', 'Kinv', 'alpha', 'info', 'trace'), new, old):
        a, b = eng.to_host(a), eng.to_host(b)
        assert a.shape == b.shape and np.array_equal(a, b), name
    assert np.all(eng.to_host(new[3])[:, 0] == n_it) and np.all(eng.to_host(new[3])[:, 3] == 0)


@pytest.mark.parametrize('m,d,flags', [(37, 1, 2), (130, 3, 3), (65, 3, 0)])
def test_trajectory_of_25_evaluations(eng, m, d, flags):
    """The trace of 25 evaluations (rel_error = 0) with the noise case, parameter by parameter, against the float64 oracle at the
    trajectory bar of tests/test_gpr_ard_gpu.py."""
    r, n_it, lr, kernel = 3, 25, 0.1, 'matern52'
    n_par = layout(d, flags)[2]
    P0, Y = gp_case(m, d, r, seed=10 + m, noise=0.3)
    w, V = noise_case(m, r, seed=1000 + m + d)
    w_d, V_d = device_noise(eng, w, V)
    raw, Kinv, alpha, info, tr = eng.gp_train_noise(eng.to_device(P0), strided(eng, Y), w_d, V_d, kernel, flags, eng.zeros((r, n_par)),
                                                    lr, n_it, 0.0, trace=True)
    tr, info, raw = eng.to_host(tr), eng.to_host(info), eng.to_host(raw)
    assert tr.shape == (r, n_it, 1 + n_par) and np.all(info[:, 0] == n_it) and np.all(info[:, 3] == 0)
    for q in range(r):
        t = gp2_train_noise(P0, Y[:, q], kernel, flags, w, V[:, q], lr=lr, max_iter=n_it, tol=0.0)
        bar, dg_max, v, b2t, worst = np.zeros(n_par), np.zeros(n_par), np.zeros(n_par), 1.0, 0.0
        for j in range(n_it):
            p = t['trace'][j, 1:]
            ev = gp2_loss_grad_noise(P0, Y[:, q], p, kernel, flags, w, V[:, q])
            rel, sc = rel_bar(ev, P0, m), noise_scales(ev, p, m, d, flags, w)
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
        print(f'trajectory m={m} d={d} flags={flags} mode {q}: max |d raw| {np.max(np.abs(tr[q, :, 1:] - t["trace"][:, 1:])):.2e} '
              f'final bar {bar.tolist()} worst ratio {worst:.2e}')
        assert np.all(np.abs(raw[q] - t['raw']) <= bar + 8 * EPS * (np.abs(t['raw']) + lr) * n_it)
        assert info[q, 1] == tr[q, -1, 0]                        # the info row holds the last evaluation with a step


@pytest.mark.parametrize('m,d,flags,seed,bar', [(37, 1, 0, 4, 1.9e-12), (130, 3, 3, 5, 6.0e-12)])
def test_retraining_to_convergence(eng, m, d, flags, seed, bar):
    """Default training (max_iter 1000, rel_error 1e-5, lr 0.1, Matern-5/2) of 5 modes on gp_case(m, d, 5, seed, noise=0.3) with
    the noise case, warm-started as GPR.update(retrain=True) starts it: from the raw values the homoscedastic oracle trains on
    the first m - k points.  The oracle stops after 15/17/22/27/21 (m = 37, plain kernel) and 32/32/50/16/18 (m = 130, ARD and
    output scale) evaluations, and its last two e lie more than 1 % away from rel_error in every mode (e / rel_error of the last
    two: m = 37 5.46/0.22, 11.49/0.87, 5.59/0.69, 2.52/0.80, 8.15/0.66;  m = 130 3.06/0.57, 10.99/0.61, 10.73/0.63, 3.25/0.21,
    4.12/0.71 -- checked on the CPU, asserted again here), so the evaluation count must be equal.  The bar on the final raw is
    MEASURED on the CPU: ten times the larger of the final differences between the float64 oracle and (a) the float64 oracle
    with K^-1 and log det from LU (route='inv'), (b) the longdouble oracle, over the five modes --
    m = 37: (a) 1.87e-13, (b) 1.62e-13 -> 1.9e-12;  m = 130: (a) 5.96e-13, (b) 4.88e-13 -> 6.0e-12."""
    r, tol, kernel = 5, 1e-5, 'matern52'
    P0, Y = gp_case(m, d, r, seed=seed, noise=0.3)
    w, V = noise_case(m, r, seed=1000 + m + d)
    k = max(1, m // 4)
    warm = np.stack([gp2_train(P0[:m - k], Y[:m - k, q], kernel, flags)['raw'] for q in range(r)])
    w_d, V_d = device_noise(eng, w, V)
    raw, Kinv, alpha, info, _ = eng.gp_train_noise(eng.to_device(P0), strided(eng, Y), w_d, V_d, kernel, flags, eng.to_device(warm), 0.1,
                                                   1000, tol)
    raw, info = eng.to_host(raw), eng.to_host(info)
    ts = [gp2_train_noise(P0, Y[:, q], kernel, flags, w, V[:, q], raw0=warm[q]) for q in range(r)]
    for q, t in enumerate(ts):
        assert abs(t['es'][-1] / tol - 1) > 0.01 and abs(t['es'][-2] / tol - 1) > 0.01 and 2 <= t['iterations'] < 1000
        print(f'retraining m={m} flags={flags} mode {q}: evaluations {int(info[q, 0])} / {t["iterations"]}, e {info[q, 2]:.3e} / '
              f'{float(t["e"]):.3e}, max |d raw| {np.max(np.abs(raw[q] - t["raw"])):.2e} (bar {bar:.1e})')
    for q, t in enumerate(ts):
        assert info[q, 3] == 0 and int(info[q, 0]) == t['iterations']
        assert np.max(np.abs(raw[q] - t['raw'])) <= bar


@pytest.mark.parametrize('flags', [0, 3])
@pytest.mark.parametrize('m', [37, 257])
def test_a_fixed_noise_equal_to_the_learned_one(eng, m, flags):
    """w = 0 on the last k rows with V = s2_q there (s2 from the host's softplus) is the homoscedastic model: K^-1, alpha and the
    loss within 2 rel of gp_train_ard at the same raw values (each is within rel of the truth; the form of
    test_flags_zero_against_the_existing_entry_point in tests/test_gpr_ard_gpu.py)."""
    d, r, kernel = 3, 3, 'matern52'
    P0, Y, raws = factor_inputs(m, r, d, flags)
    k = max(1, m // 4)
    w, V = np.ones(m), np.zeros((m, r))
    w[m - k:] = 0.0
    for q in range(r):
        V[m - k:, q] = float(split(raws[q], d, flags)[2])
    P0_d, raws_d = eng.to_device(P0), eng.to_device(raws)
    w_d, V_d = device_noise(eng, w, V)
    _, Kinv0, alpha0, info0, _ = eng.gp_train_ard(P0_d, strided(eng, Y), kernel, flags, raws_d, 0.1, 0, 0.0)
    _, Kinv1, alpha1, info1, _ = eng.gp_train_noise(P0_d, strided(eng, Y), w_d, V_d, kernel, flags, raws_d, 0.1, 0, 0.0)
    Kinv0, alpha0, info0, Kinv1, alpha1, info1 = (eng.to_host(t) for t in (Kinv0, alpha0, info0, Kinv1, alpha1, info1))
    assert info1.shape == info0.shape and np.all(info0[:, 3] == 0) and np.all(info1[:, 3] == 0)
    for q in range(r):
        ev = gp2_loss_grad(P0, Y[:, q], raws[q], kernel, flags, dtype=LD)
        rel, sc = rel_bar(ev, P0, m), scales(ev, raws[q], m, d, flags)
        errs = dict(Kinv=np.max(np.abs(Kinv1[q] - Kinv0[q])) / sc['Kinv'], alpha=np.max(np.abs(alpha1[q] - alpha0[q])) / sc['alpha'],
                    loss=abs(info1[q, 1] - info0[q, 1]) / sc['loss'])
        print(f'fixed = learned m={m} flags={flags} mode {q}: 2 x bar {2 * rel:.2e} differences ' + ' '.join(f'{k_} {v:.2e}' for k_, v in errs.items()))
        for k_, v in errs.items():
            assert v <= 2 * rel, (k_, v, rel)


def test_two_runs_agree_bit_for_bit(eng):
    m, d, r, flags = 130, 3, 5, 3
    P0, Y = gp_case(m, d, r, seed=7, noise=0.3)
    w, V = noise_case(m, r, seed=1000 + m + d)
    Ps = np.random.default_rng(1).standard_normal((70, d))
    runs = []
    for _ in range(2):
        P0_d = eng.to_device(P0)
        w_d, V_d = device_noise(eng, w, V)
        raw, Kinv, alpha, info, tr = eng.gp_train_noise(P0_d, strided(eng, Y), w_d, V_d, 'matern52', flags, eng.zeros((r, 6)), 0.1, 30,
                                                        1e-5, trace=True)
        mean, var = eng.gp_predict_ard(P0_d, eng.to_device(Ps), 'matern52', flags, raw, Kinv, alpha)
        runs.append([eng.to_host(t) for t in (raw, Kinv, alpha, info, tr, mean, var)])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    assert all(np.array_equal(K, K.T) for K in runs[0][1])


@pytest.mark.parametrize('kernel', [None, GPKernel('matern52', ard=True, scale=True)], ids=['plain', 'ard+scale'])
def test_end_to_end_against_the_oracle_driven_double(eng, kernel):
    """The public GPR on the HIP engine against the same class over the oracle-driven engine double: fit, train (30 evaluations,
    rel_error = 0: no stopping decision), update(fixed_noise=True), predict, update(retrain=True) with 30 more, predict,
    reconstruct, reconstruct_std.  As in tests/test_gpr_gpu.py and tests/test_gpr_ard_gpu.py the two sets of hyper-parameters agree
    to the 1e-11 of the trajectory bars, and coefficients and fields are smooth in them with a sensitivity of at most kappa(K):
    every output is held to 1e-11 kappa_max relative to its largest entry, the records' raw values to 1e-11 kappa_max absolutely
    (kappa_max over the three factorisations of the oracle's side).  A POD mode's sign is arbitrary between two eigensolvers:
    the measured coefficients and the constant means follow it."""
    flags = 0 if kernel is None else kernel.flags
    X, F, P = field_case()
    P_star = np.array([[2.2, 320.0], [3.3, 341.0], P[4]])
    P_new = np.array([[1.7, 333.0], [2.9, 310.0], [3.8, 349.0]])
    rng = np.random.default_rng(1)
    objs = []
    for e in (GpNoiseNumpyEngine(), eng):
        g = GPR(X, F, None, P, engine=e)
        g.fit(select_modes='number', n_modes=3)
        g.train(kernel=kernel, max_iter=30, rel_error=0.0)
        objs.append(g)
    h, g = objs
    sign = np.sign(np.sum(g.Vr * h.Vr, axis=0))
    amax = np.abs(h.Ar).max()
    A_new = h.predict(P_new)[0] + 0.05 * amax * rng.standard_normal((3, 3))
    A_sig = 0.05 * amax * (0.5 + rng.random((3, 3)))
    kappa, out = 0.0, {}

    def cond_now():
        info = h.gpr_info_
        P0_tot, Y_tot = h._d['gp_P0'].numpy(), h._d['gp_Y'].numpy()
        w, V = info.get('noise_weight', np.ones(len(P0_tot))), info.get('fixed_noise', np.zeros(Y_tot.shape))
        return max(np.linalg.cond(gp2_loss_grad_noise(P0_tot, Y_tot[:, i], np.asarray(q.raw), 'matern52', flags, w, V[:, i])['K'])
                   for i, q in enumerate(h.models))

    kappa = max(kappa, cond_now())
    for obj, s in ((h, 1.0), (g, sign)):
        obj.update(P_new, A_new * s, A_sig, fixed_noise=True)
        res = list(obj.predict(P_star))
        if obj is h:
            kappa = max(kappa, cond_now())
        obj.update(P_new, A_new * s, A_sig, retrain=True)
        A_pred, A_sigma = obj.predict(P_star)
        if obj is h:
            kappa = max(kappa, cond_now())
        res += [A_pred, A_sigma, obj.reconstruct(A_pred), obj.reconstruct_std(A_sigma)]
        out[obj is g] = res
    dev, ref = out[True], out[False]
    assert np.array_equal(g.gpr_info_['iterations'], [30, 30, 30]) and np.array_equal(h.gpr_info_['iterations'], [30, 30, 30])
    assert g.gpr_info_['n_train'] == 15 and g.Vr_sigma.shape == (15, 3) and g.gpr_info_['noise_weight'].shape == (15,)
    tol = 1e-11 * kappa
    for i, (a, b) in enumerate(zip(g.models, h.models)):
        da = a.raw - b.raw
        da[-1] = a.raw[-1] - sign[i] * b.raw[-1]                # the constant mean follows the mode's sign
        print(f'end to end mode {i}: max |d raw| {np.max(np.abs(da)):.2e}')
        assert np.max(np.abs(da)) <= tol and a.status == 0 and a.iterations == 30
    names = ('A_pred (fixed)', 'A_sigma (fixed)', 'A_pred (retrained)', 'A_sigma (retrained)', 'field', 'field std')
    dev[0], dev[2] = dev[0] * sign, dev[2] * sign
    for name, a, b in zip(names, dev, ref):
        err = np.max(np.abs(a - b)) / np.max(np.abs(b))
        print(f'end to end {name}: relative error {err:.2e} (bar {tol:.2e}, kappa {kappa:.2e})')
    for name, a, b in zip(names, dev, ref):
        assert a.shape == b.shape and np.max(np.abs(a - b)) <= tol * np.max(np.abs(b)), name
    Ad, Sd = g.predict(P_star, to_host=False)
    assert Ad.is_cuda and np.array_equal(g.reconstruct(Ad), dev[4]) and np.array_equal(g.reconstruct_std(Sd), dev[5])
