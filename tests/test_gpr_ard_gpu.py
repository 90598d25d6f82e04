"""The ARD / output-scale kernels of csrc/gp.hip on the GPU against the NumPy oracle of tests/test_gpr_ard_host.py, at the
kernel's edges rather than the workload's (the rationale of tests/test_gpr_gpu.py): the block row of 16, the LDS chunk of 32
contraction rows and the 256 threads that each own one column -- m in {1, 2, 37, 65, 130, 257} -- with (d, flags) in
{(1, scale), (3, ARD), (3, both), (8, both)} (8 = SPR_GP_MAX_D, every lengthscale slot in use), r in {1, 5}, Y with a row stride.

THE BAR of the factor-only tests (written before the first GPU run).  rel = c m eps kappa_2(K), eps = 2^-53, and
c = 16 + d + |zmax|_2:
* 12 = 3 x 4 for the four explicitly formed factors (Cholesky factor, its inverse, X^T X, K^-1 res), each with a backward error
  of about 3 m eps |K| (Higham, Accuracy and Stability, Thm 10.4): unchanged from tests/test_gpr_gpu.py, the code is shared.
* 4 + d for forming K from quantities that carry RELATIVE errors: the 4 of tests/test_gpr_gpu.py (softplus, the polynomial and
  exp of the device library, here also the product with o) plus one division and one fma per coordinate, an absolute
  perturbation of at most (4 + d) eps o per entry, |dK|_2 <= (4 + d) m eps |K|_2 since |K|_2 >= o + s2.
* |zmax|_2, zmax_c = max_i |P0[i, c]| / l_c: what a count of roundings alone (16 + d) leaves out.  The model divides BEFORE it subtracts
  (z = P0 / l, u_c = z_ic - z_jc), so u_c carries the ABSOLUTE error eps (|z_ic| + |z_jc|) / 2 <= eps zmax_c of the two rounded
  quotients, which is not small relative to t for near neighbours far from the origin (l = 0.05 puts z at 60).  Then
  |dt| <= |du|_2 <= eps |zmax|_2, |dK_ij| <= o sup|k'| |dt| <= o eps |zmax|_2 (sup |k'| <= 1 for the four kernels), and
  |dK|_2 <= m eps |zmax|_2 |K|_2.  It is computed from the inputs alone.
A backward error of rel / kappa in K moves K^-1 by rel |K^-1|_2 and alpha by rel |K^-1|_2 |res|_2, so each quantity is held to
rel times a norm bound on its sum of absolute terms (scales() below, those of tests/test_gpr_gpu.py plus two): with sK =
|K^-1|_2, sa = sK |res|_2 and |W_ij| <= sK + sa^2, the gradient of lengthscale c to sigmoid(raw_l[c]) (sK + sa^2) o sum |dk u_c^2 /
t^2| / (2 m l_c) (not ARD: o sum |dk| / (2 m l)), that of the output scale to sigmoid(raw_o) (sK + sa^2) sum |k| / 2m.  The reference
values are the oracle in np.longdouble, kappa is taken from its K.  Inputs are chosen so that rel < 1e-8 (asserted).

Trajectory bar: that of tests/test_gpr_gpu.py over n_par parameters -- a gradient error dg_c changes Adam's step by at most
2 lr dg_c / sqrt(v^_c); with dg_c = rel x the gradient's scale at evaluation i, the bar of parameter c at evaluation j is
sum_{i < j} 2 x 2 lr max_{i' <= i} dg_c / sqrt(v^_c,i) + 8 eps (|p_c| + lr) j.

Predict bar: rel times the sums of absolute terms with o in them, |mu| + o |k*|_2 sa for the mean and o + o^2 |k*|_2^2 sK + s2 for
the variance."""
import numpy as np
import pytest

from openmeasure_amd.gpr import GPR, GPKernel
from tests.test_gpr_ard_host import Gp2NumpyEngine, gp2_loss_grad, gp2_predict, gp2_train, layout, scaled_t, split, widen
from tests.test_gpr_host import KERNELS, field_case, gp_case, gp_kernel, sigmoid

pytestmark = pytest.mark.gpu
LD = np.longdouble
EPS = 2.0 ** -53
LOG_2PI = np.log(2.0 * np.pi)
F64 = lambda a: np.asarray(a, dtype=np.float64)


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


def scales(ev, raw, m, d, flags):
    """norm bounds on the sums of absolute terms (module docstring), from an oracle evaluation"""
    L, S, n_par = layout(d, flags)
    raw = F64(raw)
    sK = np.linalg.norm(F64(ev['Kinv']), 2)
    rn = np.linalg.norm(F64(ev['res']))
    sa = sK * rn
    w, o, ell, dk = sK + sa * sa, float(ev['o']), F64(ev['ell']), F64(ev['dk'])
    if flags & 1:
        gl = [float(sigmoid(raw[c])) * w * o * np.sum(np.abs(dk * F64(ev['u2'][c]) / F64(ev['t']) ** 2)) / (2 * m * ell[c]) for c in range(d)]
    else:
        gl = [float(sigmoid(raw[0])) * w * o * np.sum(np.abs(dk)) / (2 * m * ell[0])]
    go = [float(sigmoid(raw[L])) * w * np.sum(np.abs(F64(ev['k']))) / (2 * m)] if S else []
    return dict(Kinv=sK, alpha=sa, loss=(0.5 * sa * rn + 0.5 * np.sum(np.abs(F64(ev['logdiag']))) + 0.5 * m * LOG_2PI) / m,
                grad=np.array(gl + go + [float(sigmoid(raw[L + S])) * (m * sK + sa * sa) / (2 * m), sa / np.sqrt(m)]))


def rel_bar(ev, P0, m):
    """c m eps kappa with c = 16 + d + |zmax|_2 (module docstring)"""
    zmax = np.linalg.norm(np.max(np.abs(F64(P0)), axis=0) / F64(ev['ell']))
    rel = (16 + P0.shape[1] + zmax) * m * EPS * np.linalg.cond(F64(ev['K']))
    assert rel < 1e-8, rel
    return rel


FACTOR_M = [(1, 5), (2, 1), (37, 5), (65, 1), (130, 5), (257, 1)]                   # m and r, alternating
FACTOR_CASES = [(m, r, d, flags, kernel) for m, r in FACTOR_M for d, flags in ((1, 2), (3, 1), (3, 3), (8, 3))
                for kernel in (KERNELS if m in (37, 130) else ('matern52',))]


def factor_inputs(m, r, d, flags):
    P0, Y = gp_case(m, d, r, seed=m + d)
    return P0, Y, np.array([widen((q if r > 1 else m + d) % 3, d, flags) for q in range(r)])


@pytest.mark.parametrize('m,r,d,flags,kernel', FACTOR_CASES)
def test_factor_only(eng, m, r, d, flags, kernel):
    """max_iter = 0 at fixed raw (mode q takes setting q % 3 of RAWS widened to n_par; with r = 1, setting (m + d) % 3): alpha,
    K^-1, loss and every gradient component against the longdouble oracle at the bar of the module docstring."""
    P0, Y, raws = factor_inputs(m, r, d, flags)
    n_par = layout(d, flags)[2]
    raw, Kinv, alpha, info, tr = eng.gp_train_ard(eng.to_device(P0), strided(eng, Y), kernel, flags, eng.to_device(raws), 0.1, 0, 0.0)
    raw, Kinv, alpha, info = (eng.to_host(t) for t in (raw, Kinv, alpha, info))
    assert tr is None and np.array_equal(raw, raws) and info.shape == (r, 4 + n_par)
    assert np.all(info[:, 0] == 0) and np.all(info[:, 3] == 0)
    for q in range(r):
        ev = gp2_loss_grad(P0, Y[:, q], raws[q], kernel, flags, dtype=LD)
        rel, sc = rel_bar(ev, P0, m), scales(ev, raws[q], m, d, flags)
        errs = dict(Kinv=np.max(np.abs(Kinv[q] - ev['Kinv'])), alpha=np.max(np.abs(alpha[q] - ev['alpha'])),
                    loss=abs(info[q, 1] - ev['loss']))
        errs.update({f'grad{c}': abs(info[q, 4 + c] - ev['grad'][c]) for c in range(n_par)})
        bars = dict(Kinv=sc['Kinv'], alpha=sc['alpha'], loss=sc['loss'], **{f'grad{c}': sc['grad'][c] for c in range(n_par)})
        print(f'factor m={m} d={d} flags={flags} {kernel} mode {q}: bar {rel:.2e} errors / scale ' +
              ' '.join(f'{k} {float(v) / max(bars[k], 1e-300):.2e}' for k, v in errs.items()))
        assert np.array_equal(Kinv[q], Kinv[q].T)                # both halves add the same products in the same order
        for k, v in errs.items():
            assert v <= rel * bars[k], (k, float(v), rel, bars[k])


@pytest.mark.parametrize('m', [37, 257])
def test_flags_zero_against_the_existing_entry_point(eng, m):
    """The new path with neither flag is the model of spr_gp_train_f64: both on the device with the same inputs, loss, alpha and
    K^-1 within 2 rel of each other (each is within rel of the truth; not bit-equal, the distances are formed differently)."""
    d, r, kernel = 3, 3, 'matern52'
    P0, Y = gp_case(m, d, r, seed=40 + m)
    raws = np.array([widen(q % 3, d, 0) for q in range(r)])
    P0_d, raws_d = eng.to_device(P0), eng.to_device(raws)
    _, Kinv0, alpha0, info0, _ = eng.gp_train(P0_d, strided(eng, Y), kernel, raws_d, 0.1, 0, 0.0)
    _, Kinv1, alpha1, info1, _ = eng.gp_train_ard(P0_d, strided(eng, Y), kernel, 0, raws_d, 0.1, 0, 0.0)
    Kinv0, alpha0, info0, Kinv1, alpha1, info1 = (eng.to_host(t) for t in (Kinv0, alpha0, info0, Kinv1, alpha1, info1))
    assert info1.shape == (r, 7) and np.all(info0[:, 3] == 0) and np.all(info1[:, 3] == 0)
    for q in range(r):
        ev = gp2_loss_grad(P0, Y[:, q], raws[q], kernel, 0, dtype=LD)
        rel, sc = rel_bar(ev, P0, m), scales(ev, raws[q], m, d, 0)
        errs = dict(Kinv=np.max(np.abs(Kinv1[q] - Kinv0[q])) / sc['Kinv'], alpha=np.max(np.abs(alpha1[q] - alpha0[q])) / sc['alpha'],
                    loss=abs(info1[q, 1] - info0[q, 1]) / sc['loss'])
        print(f'flags 0 against gp_train m={m} mode {q}: 2 x bar {2 * rel:.2e} differences ' + ' '.join(f'{k} {v:.2e}' for k, v in errs.items()))
        for k, v in errs.items():
            assert v <= 2 * rel, (k, v, rel)


@pytest.mark.parametrize('m,d', [(37, 1), (65, 3), (130, 3)])
def test_trajectory_of_25_evaluations(eng, m, d):
    """The trace of 25 evaluations (rel_error = 0, both flags), parameter by parameter, against the float64 oracle at the
    trajectory bar of the module docstring."""
    r, n_it, lr, flags, kernel = 3, 25, 0.1, 3, 'matern52'
    n_par = layout(d, flags)[2]
    P0, Y = gp_case(m, d, r, seed=10 + m, noise=0.3)
    raw, Kinv, alpha, info, tr = eng.gp_train_ard(eng.to_device(P0), strided(eng, Y), kernel, flags, eng.zeros((r, n_par)), lr, n_it,
                                                  0.0, trace=True)
    tr, info, raw = eng.to_host(tr), eng.to_host(info), eng.to_host(raw)
    assert tr.shape == (r, n_it, 1 + n_par) and np.all(info[:, 0] == n_it) and np.all(info[:, 3] == 0)
    for q in range(r):
        t = gp2_train(P0, Y[:, q], kernel, flags, lr=lr, max_iter=n_it, tol=0.0)
        bar, dg_max, v, b2t, worst = np.zeros(n_par), np.zeros(n_par), np.zeros(n_par), 1.0, 0.0
        for j in range(n_it):
            p = t['trace'][j, 1:]
            ev = gp2_loss_grad(P0, Y[:, q], p, kernel, flags)
            rel, sc = rel_bar(ev, P0, m), scales(ev, p, m, d, flags)
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
        print(f'trajectory m={m} d={d} mode {q}: max |d raw| {np.max(np.abs(tr[q, :, 1:] - t["trace"][:, 1:])):.2e} '
              f'final bar {bar.tolist()} worst ratio {worst:.2e}')
        assert np.all(np.abs(raw[q] - t['raw']) <= bar + 8 * EPS * (np.abs(t['raw']) + lr) * n_it)
        assert info[q, 1] == tr[q, -1, 0]                        # the info row holds the last evaluation with a step


@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('m,d,n_p', [(37, 1, 1), (65, 3, 70), (2, 1, 70), (300, 3, 70)])
def test_predict_against_the_closed_form(eng, m, d, n_p, kernel):
    """mean = mu + o k*.alpha, var = max(o - o^2 k*^T K^-1 k*, 0) + s2 (both flags) against longdouble at the predict bar of the
    module docstring.  Row 0 of P_star is a training point; with n_p = 70, row 1 lies 1000 units away: every kernel underflows
    to 0 there, the mean is mu and the variance o + s2 to rounding (that row is left out of zmax: its k* is 0 whatever its z)."""
    r, flags = 3, 3
    P0, Y = gp_case(m, d, r, seed=20 + m)
    raws = np.array([widen(q % 3, d, flags) for q in range(r)])
    rng = np.random.default_rng(m)
    Ps = rng.standard_normal((n_p, d)) * 1.5
    Ps[0] = P0[min(3, m - 1)]
    if n_p > 1:
        Ps[1] = P0.mean(axis=0) + 1000.0
    P0_d = eng.to_device(P0)
    raw, Kinv, alpha, info, _ = eng.gp_train_ard(P0_d, eng.to_device(Y), kernel, flags, eng.to_device(raws), 0.1, 0, 0.0)
    mean, var = eng.gp_predict_ard(P0_d, eng.to_device(Ps), kernel, flags, raw, Kinv, alpha)
    mean, var = eng.to_host(mean), eng.to_host(var)
    assert mean.shape == var.shape == (n_p, r)
    evs = [gp2_loss_grad(P0, Y[:, q], raws[q], kernel, flags, dtype=LD) for q in range(r)]
    want_m, want_v = gp2_predict(P0.astype(LD), Ps.astype(LD), raws.astype(LD), np.stack([e['Kinv'] for e in evs]),
                                 np.stack([e['alpha'] for e in evs]), kernel, flags)
    worst = 0.0
    for q in range(r):
        rel, sc = rel_bar(evs[q], np.concatenate([P0, Ps[:1], Ps[2:]]), m), scales(evs[q], raws[q], m, d, flags)
        ell, o, s2, mu = (F64(x) for x in split(raws[q], d, flags))
        kn = np.linalg.norm(gp_kernel(kernel, scaled_t(Ps / ell, P0 / ell)[0])[0], axis=1)
        em = np.abs(mean[:, q] - want_m[:, q]) / (abs(mu) + o * kn * sc['alpha'] + 1e-300)
        evr = np.abs(var[:, q] - want_v[:, q]) / (o + o * o * kn * kn * sc['Kinv'] + s2)
        worst = max(worst, float(np.max(em)) / rel, float(np.max(evr)) / rel)
        assert np.all(em <= rel) and np.all(evr <= rel), (q, float(np.max(em)), float(np.max(evr)), rel)
        assert np.all(var[:, q] >= s2 * (1 - 4 * EPS))
        if n_p > 1:
            assert abs(var[1, q] - (o + s2)) <= 4 * EPS * (o + s2) and abs(mean[1, q] - mu) <= EPS * abs(mu)
    print(f'predict m={m} d={d} n_p={n_p} {kernel}: worst error / bar {worst:.2e}')


def test_two_runs_agree_bit_for_bit(eng):
    m, d, r, flags = 130, 3, 5, 3
    P0, Y = gp_case(m, d, r, seed=7, noise=0.3)
    Ps = np.random.default_rng(1).standard_normal((70, d))
    runs = []
    for _ in range(2):
        P0_d = eng.to_device(P0)
        raw, Kinv, alpha, info, tr = eng.gp_train_ard(P0_d, strided(eng, Y), 'matern52', flags, eng.zeros((r, 6)), 0.1, 30, 1e-5,
                                                      trace=True)
        mean, var = eng.gp_predict_ard(P0_d, eng.to_device(Ps), 'matern52', flags, raw, Kinv, alpha)
        runs.append([eng.to_host(t) for t in (raw, Kinv, alpha, info, tr, mean, var)])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    assert all(np.array_equal(K, K.T) for K in runs[0][1])


def test_end_to_end_against_the_oracle_driven_double(eng):
    """The public GPR with GPKernel('matern52', ard=True, scale=True) on the HIP engine against the same class over the
    oracle-driven engine double, after 30 evaluations (rel_error = 0: no stopping decision).  As in tests/test_gpr_gpu.py the two
    sets of hyper-parameters agree to the 1e-11 of the trajectory bars, and coefficients and fields are smooth in them with a
    sensitivity of at most kappa(K): every output is held to 1e-11 kappa_max relative to its largest entry, the records' raw
    values to 1e-11 kappa_max absolutely."""
    X, F, P = field_case()
    gk = GPKernel('matern52', ard=True, scale=True)
    P_star = np.array([[2.2, 320.0], [3.3, 341.0], P[4]])
    out = []
    for e in (eng, Gp2NumpyEngine()):
        g = GPR(X, F, None, P, engine=e)
        g.fit(select_modes='number', n_modes=3)
        g.train(kernel=gk, max_iter=30, rel_error=0.0)
        A_pred, A_sigma = g.predict(P_star)
        out.append((g, A_pred, A_sigma, g.reconstruct(A_pred), g.reconstruct_std(A_sigma)))
    (g, *dev), (h, *ref) = out
    assert np.array_equal(g.gpr_info_['iterations'], [30, 30, 30]) and np.array_equal(h.gpr_info_['iterations'], [30, 30, 30])
    assert g.gpr_info_['grad'].shape == (3, 5) and g.gpr_info_['lengthscale'].shape == (3, 2) and g.Vr_sigma.shape == (12, 3)
    sign = np.sign(np.sum(g.Vr * h.Vr, axis=0))                # a POD mode's sign is arbitrary between two eigensolvers
    kappa = max(np.linalg.cond(gp2_loss_grad(h.P0, h.Vr[:, i], q.raw, 'matern52', 3)['K']) for i, q in enumerate(h.models))
    tol = 1e-11 * kappa
    for i, (a, b) in enumerate(zip(g.models, h.models)):
        da = a.raw - b.raw
        da[-1] = a.raw[-1] - sign[i] * b.raw[-1]                # the constant mean follows the mode's sign
        print(f'end to end mode {i}: max |d raw| {np.max(np.abs(da)):.2e}, lengthscale {a.lengthscale.tolist()}, outputscale {a.outputscale:.4f}')
        assert np.max(np.abs(da)) <= tol and a.status == 0 and a.iterations == 30
        assert isinstance(a.lengthscale, np.ndarray) and a.lengthscale.shape == (2,) and isinstance(a.outputscale, float)
    names = ('A_pred', 'A_sigma', 'field', 'field std')
    dev[0] = dev[0] * sign
    for name, a, b in zip(names, dev, ref):
        err = np.max(np.abs(a - b)) / np.max(np.abs(b))
        print(f'end to end {name}: relative error {err:.2e} (bar {tol:.2e}, kappa {kappa:.2e})')
    for name, a, b in zip(names, dev, ref):
        assert a.shape == b.shape and np.max(np.abs(a - b)) <= tol * np.max(np.abs(b)), name
    # the device tensors of predict(to_host=False) go straight into reconstruct / reconstruct_std
    Ad, Sd = g.predict(P_star, to_host=False)
    assert Ad.is_cuda and np.array_equal(g.reconstruct(Ad), dev[2]) and np.array_equal(g.reconstruct_std(Sd), dev[3])
