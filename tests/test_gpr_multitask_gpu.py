"""spr_gp_train_mt_f64 / spr_gp_predict_mt_f64 (csrc/gp.hip; engine.gp_train_mt, gp_predict_mt; GPR(gpr_type='MultiTask')) on the GPU
against the NumPy oracle of tests/test_gpr_multitask_host.py: the evaluation kernel at the edges of the shared factorisation (the
block row of 16, the LDS chunk of 32, the 256 columns: m in {1, 2, 37, 65, 130, 257}, d in {1, 3}, r in {1, 5}, flags 0 and 3, Y
with a row stride), the step kernel's own edges (one parameter vector of 4, 271 and 331 values: more than one pass of 256 threads),
the trajectory, the stopping decision, the launch chain at the chunk length, and the public class.

THE BARS (written before the first GPU run).
Per-mode quantities: those of tests/test_gpr_gpu.py, rel_q = 16 m eps kappa_2(K_q) (its rel_bar, imported; K_q includes the task
and the global noise), times the norm bounds of the sums of absolute terms -- scales() of tests/test_gpr_ard_gpu.py, which are
those of tests/test_gpr_gpu.py written for n_par parameters (sK = |K^-1|_2, sa = sK |res|_2; the loss, each lengthscale, the output
scale, the noise sigmoid(raw_t) (m sK + sa^2) / 2m, the mean sa / sqrt(m)).
Joint quantities follow from them, with (r + 2) eps of the summed magnitudes for the r-term sum, its division and one product:
* LOSS: mean_q rel_q loss-scale_q + (r + 2) eps mean_q |loss_q|.
* own parameters of mode q: rel_q x the per-mode gradient scale / r (the division by r is one rounding of a value below the scale:
  it is inside the 16).
* d / d raw_g: sigmoid(raw_g) (1 / r) sum_q rel_q (m sK_q + sa_q^2) / 2m + (r + 2) eps sigmoid(raw_g) (1 / r) sum_q |tw_q|.
Against spr_gp_train_noise_f64 (max_iter = 0, w = 1, V = softplus(raw_g) + 1e-4): K^-1, alpha, the per-mode loss (through LOSS, the
sum in index order divided by r, formed on the host from the single-task losses with the same IEEE operations) and the own
gradients (the single-task ones divided by r) are EQUAL, bit for bit: the same device function on the same diagonal.
Trajectory: the accumulation rule of tests/test_gpr_gpu.py per parameter, the shared one included -- a gradient error dg_c changes
Adam's step by at most 2 lr dg_c / sqrt(v^_c); the bar of parameter c at evaluation j is sum_{i < j} 2 x 2 lr max_{i' <= i} dg_c /
sqrt(v^_c,i) + 8 eps (|p_c| + lr) j with dg_c the joint gradient bars above; LOSS at evaluation j is held to its bar plus
sum_c |g_c| bar_c,j.
Final parameters after convergence: MEASURED on the CPU, ten times the larger of the final differences (over raw and raw_g) between
the float64 oracle and (a) its LU route, (b) the longdouble oracle:
  (m, d, seed, tol) = (37, 1, 5, 1e-5):   115 evaluations, (a) 2.34e-13, (b) 1.72e-13 -> 2.4e-12
                      (130, 3, 4, 1e-3):   96 evaluations, (a) 5.72e-13, (b) 5.54e-13 -> 5.8e-12
                      (257, 3, 7, 1e-4):  122 evaluations, (a) 1.96e-12, (b) 1.01e-12 -> 2.0e-11
(e / tol of the last two evaluations: 1.342 / 0.904, 1.149 / 0.941, 1.011 / 0.981 by all three routes.)
Public class: the form of the end-to-end tests of tests/test_gpr_gpu.py -- hyper-parameters to 1e-11 kappa_max absolutely, every
output to 1e-11 kappa_max relative to its largest entry, kappa_max over the factorisations of the oracle's side."""
import pickle

import numpy as np
import pytest

from openmeasure_amd.gpr import GPR, GPKernel
from tests.test_gpr_ard_gpu import factor_inputs, scales, strided
from tests.test_gpr_ard_host import layout
from tests.test_gpr_gpu import rel_bar
from tests.test_gpr_host import KERNELS, field_case, gp_case, sigmoid, softplus
from tests.test_gpr_multitask_host import (CONVERGENCE_CASES, GpMtNumpyEngine, gp_mt_loss_grad, gp_mt_predict, gp_mt_train,
                                           recorded_convergence)

pytestmark = pytest.mark.gpu
LD = np.longdouble
EPS = 2.0 ** -53
F64 = lambda a: np.asarray(a, dtype=np.float64)


@pytest.fixture(scope='module')
def eng():
    from openmeasure_amd.engine import HipEngine
    return HipEngine('cuda:0')


def host(eng, *ts):
    return [None if t is None else eng.to_host(t) for t in ts]


def joint_bars(ev, raw, raw_g, m, d, flags):
    """-> (bar of LOSS, bars of the gradient (NP,)) from an oracle evaluation ev = gp_mt_loss_grad(...) (module docstring)"""
    r = len(raw)
    n_par = layout(d, flags)[2]
    sg = float(sigmoid(np.float64(raw_g)))
    loss_bar, g_bar, gg = 0.0, [], 0.0
    for q in range(r):
        e = ev['evs'][q]
        rel, sc = rel_bar(e, m), scales(e, raw[q], m, d, flags)
        loss_bar += rel * sc['loss']
        g_bar.append(rel * sc['grad'] / r)
        gg += rel * (m * sc['Kinv'] + sc['alpha'] ** 2) / (2 * m)
    loss_bar = loss_bar / r + (r + 2) * EPS * float(np.mean(np.abs(F64(ev['loss_q']))))
    gg = sg * gg / r + (r + 2) * EPS * sg * float(np.mean(np.abs(F64(ev['tw']))))
    return loss_bar, np.concatenate(g_bar + [[gg]])


# ------------------------------------------------------------------------------------------------ 1. the evaluation
RAW_G = -4.0
EVAL_M = [(1, 5), (2, 1), (37, 5), (65, 1), (130, 5), (257, 1)]                      # m and r, alternating
EVAL_CASES = [(m, r if d == 3 else 6 - r, d, flags, kernel) for m, r in EVAL_M for d in (1, 3) for flags in (0, 3)
              for kernel in (KERNELS if (m, d, flags) == (37, 3, 3) else ('matern52',))]


@pytest.mark.parametrize('m,r,d,flags,kernel', EVAL_CASES)
def test_evaluation_is_the_noise_kernel_s_and_the_joint_sums(eng, m, r, d, flags, kernel):
    """max_iter = 0 at fixed raw (the settings of tests/test_gpr_ard_gpu.factor_inputs) and raw_g = -4: bit for bit against
    gp_train_noise(max_iter=0) with w = 1, V = softplus(raw_g) + 1e-4, and LOSS and the joint gradient against the longdouble
    oracle at the bars of the module docstring."""
    P0, Y, raws = factor_inputs(m, r, d, flags)
    n_par = layout(d, flags)[2]
    NP = r * n_par + 1
    P0_d, Y_d, raws_d = eng.to_device(P0), strided(eng, Y), eng.to_device(raws)
    out = eng.gp_train_mt(P0_d, Y_d, kernel, flags, raws_d, eng.to_device(np.array([RAW_G])), 0.1, 0, 0.0)
    raw, raw_g, s2, Kinv, alpha, info, tr = host(eng, *out)
    assert tr is None and np.array_equal(raw, raws) and raw_g[0] == RAW_G and info.shape == (4 + NP + r,)
    assert info[0] == 0 and np.isnan(info[2]) and info[3] == 0 and np.all(info[4 + NP:] == 0)
    vg = float(softplus(np.float64(RAW_G))) + 1e-4
    V = np.full((m, r), vg)
    _, Kinv1, alpha1, info1, _ = host(eng, *eng.gp_train_noise(P0_d, Y_d, eng.to_device(np.ones(m)), strided(eng, V, pad=2), kernel,
                                                                flags, raws_d, 0.1, 0, 0.0))
    assert np.all(info1[:, 3] == 0)
    assert np.array_equal(Kinv, Kinv1) and np.array_equal(alpha, alpha1)
    LOSS = 0.0
    for q in range(r):
        LOSS = LOSS + info1[q, 1]
    assert info[1] == LOSS / r
    assert np.array_equal(info[4:4 + NP - 1].reshape(r, n_par), info1[:, 4:] / r)
    ev = gp_mt_loss_grad(P0, Y, raws, RAW_G, kernel, flags, dtype=LD)
    assert np.all(np.abs(s2 - F64(ev['s2'])) <= 4 * EPS * s2)
    loss_bar, g_bar = joint_bars(ev, raws, RAW_G, m, d, flags)
    dl, dg = abs(info[1] - ev['loss']), np.abs(info[4:4 + NP] - ev['grad'])
    print(f'evaluation m={m} r={r} d={d} flags={flags} {kernel}: LOSS error / bar {float(dl) / loss_bar:.2e}, gradient '
          f'{float(np.max(dg[:-1] / np.maximum(g_bar[:-1], 1e-300))):.2e}, raw_g {float(dg[-1]) / max(g_bar[-1], 1e-300):.2e}')
    assert dl <= loss_bar, (float(dl), loss_bar)
    assert np.all(dg <= g_bar), (F64(dg), g_bar)
    for q in range(r):
        assert np.array_equal(Kinv[q], Kinv[q].T)


# ------------------------------------------------------------------------------------------------ 2., 3. steps and trajectory
def check_trajectory(eng, m, d, r, flags, n_it, seed):
    lr, kernel = 0.1, 'matern52'
    n_par = layout(d, flags)[2]
    NP = r * n_par + 1
    P0, Y = gp_case(m, d, r, seed=seed, noise=0.3)
    out = eng.gp_train_mt(eng.to_device(P0), strided(eng, Y), kernel, flags, eng.zeros((r, n_par)), eng.zeros((1,)), lr, n_it, 0.0,
                          trace=True)
    raw, raw_g, s2, Kinv, alpha, info, tr = host(eng, *out)
    assert tr.shape == (n_it, 1 + NP) and info[0] == n_it and info[3] == 0 and np.all(info[4 + NP:] == 0)
    t = gp_mt_train(P0, Y, kernel, flags, lr=lr, max_iter=n_it, tol=0.0)
    bar, dg_max, v, b2t, worst = np.zeros(NP), np.zeros(NP), np.zeros(NP), 1.0, 0.0
    for j in range(n_it):
        p = t['trace'][j, 1:]
        ev = gp_mt_loss_grad(P0, Y, p[:-1].reshape(r, n_par), p[-1], kernel, flags)
        loss_bar, g_bar = joint_bars(ev, p[:-1].reshape(r, n_par), p[-1], m, d, flags)
        dp = np.abs(tr[j, 1:] - p)
        dl = abs(tr[j, 0] - t['trace'][j, 0])
        bar_j = bar + 8 * EPS * (np.abs(p) + lr) * j
        worst = max(worst, float(np.max(dp / np.maximum(bar_j, 1e-300))) if j else 0.0)
        assert np.all(dp <= bar_j), (j, dp, bar_j)
        assert dl <= loss_bar + np.sum(np.abs(ev['grad']) * bar_j), (j, dl)
        dg_max = np.maximum(dg_max, g_bar)
        b2t *= 0.999
        v = 0.999 * v + 0.001 * ev['grad'] ** 2
        bar = bar + 2 * 2 * lr * dg_max / np.sqrt(v / (1 - b2t))
    final = np.concatenate([t['raw'].ravel(), [t['raw_g']]])
    got = np.concatenate([raw.ravel(), raw_g])
    print(f'trajectory m={m} d={d} r={r} flags={flags}: max |d raw| {np.max(np.abs(tr[:, 1:] - t["trace"][:, 1:])):.2e} '
          f'largest final bar {bar.max():.2e} worst ratio {worst:.2e}')
    assert np.all(np.abs(got - final) <= bar + 8 * EPS * (np.abs(final) + lr) * n_it)
    fin = t['final']
    loss_bar, g_bar = joint_bars(fin, t['raw'], t['raw_g'], m, d, flags)
    assert abs(info[1] - fin['loss']) <= loss_bar + np.sum(np.abs(fin['grad']) * bar)      # the final evaluation, at the values kept
    assert info[2] == abs(tr[-1, 0] - tr[-2, 0])


@pytest.mark.parametrize('m,d,r,flags', [(5, 1, 1, 0), (5, 1, 90, 0), (5, 8, 30, 3)])
def test_step_kernel_edges(eng, m, d, r, flags):
    """three evaluations at tol = 0: 4, 271 and 331 parameters -- one thread's worth, and more than one pass of the 256 threads"""
    check_trajectory(eng, m, d, r, flags, 3, seed=3 + r)


@pytest.mark.parametrize('m,d', [(37, 1), (130, 3)])
def test_trajectory_of_25_evaluations(eng, m, d):
    check_trajectory(eng, m, d, 3, 0, 25, seed=10 + m)


# ------------------------------------------------------------------------------------------------ 4. convergence
@pytest.mark.parametrize('case,bar', list(zip(CONVERGENCE_CASES, (2.4e-12, 5.8e-12, 2.0e-11))))
def test_training_to_convergence(eng, case, bar):
    """The evaluation count equals the oracle's and the final parameters lie within the measured bar (module docstring).  The
    oracle's last two e lie more than 1 % from rel_error by the Cholesky route (computed here) and by the LU and longdouble routes
    (recorded in tests/golden/gpr_multitask_convergence.json; tests/test_gpr_multitask_host.py keeps the record honest)."""
    m, d, seed, tol = case
    P0, Y = gp_case(m, d, 5, seed, noise=0.3)
    t = gp_mt_train(P0, Y, 'matern52', 0, lr=0.1, max_iter=1000, tol=tol)
    for route, es, its in [('chol', t['es'][-2:], t['iterations'])] + [(ro, recorded_convergence(m, ro)['es'],
                                                                        int(recorded_convergence(m, ro)['iterations']))
                                                                       for ro in ('chol', 'inv', 'ld')]:
        assert its == t['iterations'] < 1000 and abs(es[-1] / tol - 1) > 0.01 and abs(es[-2] / tol - 1) > 0.01, (route, es, its)
    out = eng.gp_train_mt(eng.to_device(P0), strided(eng, Y), 'matern52', 0, eng.zeros((5, 3)), eng.zeros((1,)), 0.1, 1000, tol)
    raw, raw_g, s2, Kinv, alpha, info, _ = host(eng, *out)
    diff = max(np.max(np.abs(raw - t['raw'])), abs(raw_g[0] - t['raw_g']))
    print(f'convergence m={m}: evaluations {int(info[0])} / {t["iterations"]}, e {info[2]:.3e} / {float(t["e"]):.3e}, '
          f'max |d raw| {diff:.2e} (bar {bar:.1e})')
    assert info[3] == 0 and int(info[0]) == t['iterations'] and info[2] <= tol
    assert diff <= bar


# ------------------------------------------------------------------------------------------------ 5. the launch chain
def chain_case():
    """gp_case(37, 1, 3, 5): the joint loop warm-started where 60 evaluations of the oracle (lr 0.1) left it, continued with lr 0.02:
    there e falls by about 4 % per evaluation from the second on (checked on the CPU, asserted on the device's own trace), so a
    tolerance equal to e of evaluation n stops the loop exactly there"""
    P0, Y = gp_case(37, 1, 3, 5, noise=0.3)
    w = gp_mt_train(P0, Y, 'matern52', 0, max_iter=60, tol=0.0)
    return P0, Y, w['raw'], np.array([w['raw_g']])


def test_chunk_boundaries_of_the_launch_chain(eng):
    """Runs that stop after C - 1, C and C + 1 evaluations by max_iter (tol = 0) equal, bit for bit, runs with max_iter = 1000 that a
    tolerance stops at the same evaluation; the final K^-1 / alpha / s2 equal a max_iter = 0 call at the returned parameters; two
    identical runs agree bit for bit."""
    C = eng.GP_MT_CHUNK
    P0, Y, raw0, rawg0 = chain_case()
    P0_d, Y_d = eng.to_device(P0), strided(eng, Y)
    run = lambda max_iter, tol: host(eng, *eng.gp_train_mt(P0_d, Y_d, 'matern52', 0, eng.to_device(raw0), eng.to_device(rawg0), 0.02,
                                                           max_iter, tol, trace=True))
    for n in (C - 1, C, C + 1):
        a = run(n, 0.0)
        es = np.abs(np.diff(a[6][:, 0]))                        # e of evaluations 2 .. n, formed as the device forms it
        assert a[5][0] == n and a[5][2] == es[-1] and es[-1] < es[:-1].min(), (n, es)
        b = run(1000, float(es[-1]))
        assert b[5][0] == n
        for name, x, y in zip(('raw', 'raw_g', 's2', 'Kinv', 'alpha', 'info'), a, b):
            assert np.array_equal(x, y), (n, name)
        assert np.array_equal(a[6], b[6][:n]) and np.all(b[6][n:] == 0)
        c = run(n, 0.0)
        for x, y in zip(a, c):
            assert np.array_equal(x, y)
        z = host(eng, *eng.gp_train_mt(P0_d, Y_d, 'matern52', 0, eng.to_device(a[0]), eng.to_device(a[1]), 0.02, 0, 0.0))
        assert np.array_equal(z[0], a[0]) and np.array_equal(z[1], a[1])
        for name, k in (('s2', 2), ('Kinv', 3), ('alpha', 4)):
            assert np.array_equal(z[k], a[k]), (n, name)
        NP = a[0].size + 1
        assert z[5][1] == a[5][1] and np.array_equal(z[5][4:4 + NP], a[5][4:4 + NP])      # LOSS and gradient of the final evaluation


def test_a_failed_pivot_ends_the_loop_with_that_mode_s_status(eng):
    """raw_t = NaN in mode 1 of 3 makes its first pivot NaN: status 2 for that mode alone, no evaluation counted, the parameters as
    given -- a status, not a device fault; the class raises numpy.linalg.LinAlgError naming the mode."""
    P0, Y = gp_case(37, 1, 3, seed=3)
    raws = np.zeros((3, 3))
    raws[1, 1] = np.nan
    out = eng.gp_train_mt(eng.to_device(P0), eng.to_device(Y), 'matern52', 0, eng.to_device(raws), eng.zeros((1,)), 0.1, 40, 0.0)
    raw, raw_g, s2, Kinv, alpha, info, _ = host(eng, *out)
    NP = 10
    assert info[0] == 0 and info[3] == 2 and np.array_equal(info[4 + NP:], [0, 2, 0])
    assert np.array_equal(raw, raws, equal_nan=True) and raw_g[0] == 0.0
    X, F, P = field_case()
    g = GPR(X, F, None, P, gpr_type='MultiTask', engine=eng)
    g.fit(select_modes='number', n_modes=3)
    g.train(max_iter=2)
    bad = g._d['gp_raw'].clone()
    bad[1, 1] = float('nan')
    g._d['gp_raw'] = bad
    with pytest.raises(np.linalg.LinAlgError, match=r'mode\(s\) \[2\]'):
        g.update(np.array([[2.0, 320.0]]), np.ones((1, 3)))


# ------------------------------------------------------------------------------------------------ 6. the public class
@pytest.mark.parametrize('kernel', [None, GPKernel('matern52', ard=True, scale=True)], ids=['plain', 'ard+scale'])
def test_end_to_end_against_the_oracle_driven_double(eng, kernel):
    """fit, train (30 evaluations, rel_error = 0: no stopping decision), predict, update, predict, update(retrain=True) with 30
    more, predict, reconstruct, reconstruct_std and a pickle round trip, on the HIP engine and on the oracle-driven double.  A POD
    mode's sign is arbitrary between two eigensolvers: the measured coefficients and the constant means follow it."""
    flags = 0 if kernel is None else kernel.flags
    X, F, P = field_case()
    P_star = np.array([[2.2, 320.0], [3.3, 341.0], P[4]])
    P_new = np.array([[1.7, 333.0], [2.9, 310.0], [3.8, 349.0]])
    rng = np.random.default_rng(1)
    objs = []
    for e in (GpMtNumpyEngine(), eng):
        g = GPR(X, F, None, P, gpr_type='MultiTask', engine=e)
        g.fit(select_modes='number', n_modes=3)
        g.train(kernel=kernel, max_iter=30, rel_error=0.0)
        objs.append(g)
    h, g = objs
    sign = np.sign(np.sum(g.Vr * h.Vr, axis=0))
    A_new = h.predict(P_new)[0] + 0.05 * np.abs(h.Ar).max() * rng.standard_normal((3, 3))

    def cond_now():
        rec = h.models[0]
        ev = gp_mt_loss_grad(h._d['gp_P0'].numpy(), h._d['gp_Y'].numpy(), rec.raw, rec.raw_noise, 'matern52', flags)
        return max(np.linalg.cond(e['K']) for e in ev['evs'])

    kappa, out = cond_now(), {}
    for obj, s in ((h, 1.0), (g, sign)):
        res = list(obj.predict(P_star))
        obj.update(P_new, A_new * s)
        res += list(obj.predict(P_star))
        if obj is h:
            kappa = max(kappa, cond_now())
        obj.update(P_new, A_new * s, retrain=True)
        if obj is h:
            kappa = max(kappa, cond_now())
        obj2 = pickle.loads(pickle.dumps(obj))
        obj2._eng = obj._eng
        A_pred, A_sigma = obj2.predict(P_star)
        assert np.array_equal(A_pred, obj.predict(P_star)[0]) and np.array_equal(A_sigma, obj.predict(P_star)[1])
        res += [A_pred, A_sigma, obj.reconstruct(A_pred), obj.reconstruct_std(A_sigma)]
        out[obj is g] = res
    dev, ref = out[True], out[False]
    assert g.gpr_info_['iterations'] == 30 == h.gpr_info_['iterations'] and g.gpr_info_['n_train'] == 15
    assert len(g.models) == 1 and g.models[0] is g.likelihoods[0] and g.Vr_sigma.shape == (15, 3)
    tol = 1e-11 * kappa
    a, b = g.models[0], h.models[0]
    da = a.raw - b.raw
    da[:, -1] = a.raw[:, -1] - sign * b.raw[:, -1]               # the constant means follow the modes' signs
    print(f'end to end: max |d raw| {np.max(np.abs(da)):.2e}, |d raw_g| {abs(a.raw_noise - b.raw_noise):.2e} (bar {tol:.2e})')
    assert np.max(np.abs(da)) <= tol and abs(a.raw_noise - b.raw_noise) <= tol and np.all(a.status == 0)
    names = ('A_pred', 'A_sigma', 'A_pred (updated)', 'A_sigma (updated)', 'A_pred (retrained)', 'A_sigma (retrained)', 'field',
             'field std')
    for k in (0, 2, 4):
        dev[k] = dev[k] * sign
    for name, x, y in zip(names, dev, ref):
        print(f'end to end {name}: relative error {np.max(np.abs(x - y)) / np.max(np.abs(y)):.2e} (bar {tol:.2e}, kappa {kappa:.2e})')
    for name, x, y in zip(names, dev, ref):
        assert x.shape == y.shape and np.max(np.abs(x - y)) <= tol * np.max(np.abs(y)), name
    Ad, Sd = g.predict(P_star, to_host=False)
    assert Ad.is_cuda and np.array_equal(g.reconstruct(Ad), dev[6]) and np.array_equal(g.reconstruct_std(Sd), dev[7])


def test_predict_adds_the_stored_noise(eng):
    """var at a point 1000 units away is o + s2 with s2 the stored sum, bit for bit the value the last evaluation used; the mean
    there is mu; against the longdouble closed form elsewhere (rel of the module docstring times o + o^2 |k*|^2 sK + s2)."""
    m, d, r, flags, kernel = 65, 3, 5, 3, 'matern52'
    P0, Y, raws = factor_inputs(m, r, d, flags)
    P0_d = eng.to_device(P0)
    out = eng.gp_train_mt(P0_d, strided(eng, Y), kernel, flags, eng.to_device(raws), eng.to_device(np.array([RAW_G])), 0.1, 0, 0.0)
    Ps = np.random.default_rng(m).standard_normal((19, d)) * 1.5
    Ps[1] = P0.mean(axis=0) + 1000.0
    mean, var = host(eng, *eng.gp_predict_mt(P0_d, eng.to_device(Ps), kernel, flags, out[0], out[2], out[3], out[4]))
    s2 = eng.to_host(out[2])
    ev = gp_mt_loss_grad(P0, Y, raws, RAW_G, kernel, flags, dtype=LD)
    want_m, want_v = gp_mt_predict(P0.astype(LD), Ps.astype(LD), raws.astype(LD), ev['s2'], ev['Kinv'], ev['alpha'], kernel, flags)
    for q in range(r):
        e = ev['evs'][q]
        o = float(e['o'])
        rel, sc = rel_bar(e, m), scales(e, raws[q], m, d, flags)
        assert var[1, q] == o + s2[q] or abs(var[1, q] - (o + s2[q])) <= 4 * EPS * (o + s2[q])
        assert abs(mean[1, q] - raws[q, -1]) <= EPS * abs(raws[q, -1])
        kn2 = m                                                  # |k*|_2^2 <= m: k <= 1
        assert np.all(np.abs(var[:, q] - F64(want_v[:, q])) <= rel * (o + o * o * kn2 * sc['Kinv'] + s2[q]))
        assert np.all(np.abs(mean[:, q] - F64(want_m[:, q])) <= rel * (abs(raws[q, -1]) + o * np.sqrt(kn2) * sc['alpha']))
