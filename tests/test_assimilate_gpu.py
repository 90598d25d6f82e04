"""SPR.assimilate on the HIP engine: the kernels of csrc/assimilate.hip against the longdouble Kalman-form oracle of
tests/test_assimilate_host.py, at the smallest shapes where they can go wrong -- the tile edges of the 16 x 16 x 4 MFMA
Gram (s and r around 16 and 32), the panel tails (s not a multiple of the 32 or 16 sensors of a panel), every rung of the
padded width (q + 1 <= 16, 32, 48, 80, 144: q on both sides of 15|16, 31|32, 47|48, 79|80), r = 128 where the factor fills
the LDS, fewer sensors than modes, more vectors than one wave of workgroups.

Bars, per vector, with eps = 2^-52 and kappa = cond_2(H') from the ORACLE's matrices (never the device's estimate):
    |z - z_ref|_2 <= 16 (s + q) eps kappa |z_ref|_2         (z: the engine's fifth output, Ar = a0 + C z)
    |F F^T - cov_ref|_F <= the same multiple of |cov_ref|_F
    |chi2 - ref| <= the same multiple of |W res|^2,   |logdet - ref| <= the same multiple of q + sum |log sig0^2|
and Ar against a0 + C z_ref at the z bar times |C|_2 plus 2 eps |Ar| for forming it.  Inputs are drawn with kappa <= 1e8
(asserted), so the loosest bar is below 1e-4: a wrong tile, panel tail or scale shows at O(1).
Every case prints its worst error / bar ratio."""
import numpy as np
import pytest

from tests.test_assimilate_host import EPS, LD, bar_factor, check_vector, kalman_oracle

pytestmark = pytest.mark.gpu
SCALE = np.array([1.0, 25.0, 0.04])                          # three features with different scl


@pytest.fixture(scope='module')
def eng():
    from openmeasure_amd.engine import HipEngine
    return HipEngine('cuda:0')


def draw(s, r, n_p, q=None, seed=0, zero_rows=False):
    """Theta, cnt, y (n_p, s, 3), a0, and sigma (n_p, r) [q None] or factors (n_p, r, q); readings consistent with the prior"""
    rng = np.random.default_rng(seed)
    Theta = rng.standard_normal((s, r)) / np.sqrt(r)
    cnt = rng.standard_normal(s)
    a0 = rng.standard_normal((n_p, r))
    if q is None:
        prior = rng.uniform(0.3, 2.0, (n_p, r))
        if zero_rows:
            prior[0, ::3] = 0.0
            prior[-1, :] = 0.0 if n_p > 1 else prior[-1, :]
        Cs = [np.diag(p) for p in prior]
    else:
        prior = np.stack([np.linalg.qr(rng.standard_normal((r, q)))[0] * rng.uniform(0.5, 2.0, q) for _ in range(n_p)])
        if zero_rows:
            prior[0, ::3, :] = 0.0
        Cs = list(prior)
    y = np.empty((n_p, s, 3))
    for p in range(n_p):
        fid = rng.integers(0, 3, s)
        sig0 = 0.05 * rng.uniform(0.5, 2.0, s)
        y0 = Theta @ (a0[p] + Cs[p] @ rng.standard_normal(Cs[p].shape[1])) + sig0 * rng.standard_normal(s)
        y[p] = np.stack([y0 * SCALE[fid] + cnt, sig0 * SCALE[fid], fid.astype(float)], axis=1)
    return Theta, cnt, y, a0, prior, Cs


def run(eng, Theta, cnt, y, a0, prior, diag, Theta_d=None, y_d=None):
    """one engine call, repeated: two runs agree bit for bit -> host (Ar, Ar_std, F, info, z)"""
    args = (eng.to_device(Theta) if Theta_d is None else Theta_d, eng.to_device(cnt), eng.to_device(SCALE),
            eng.to_device(y) if y_d is None else y_d, eng.to_device(a0))
    kw = {'S' if diag else 'L': eng.to_device(prior)}
    out = [eng.to_host(t).copy() for t in eng.assimilate(*args, **kw)]
    again = [eng.to_host(t) for t in eng.assimilate(*args, **kw)]
    for a, b in zip(out, again):
        assert np.array_equal(a, b)                           # no atomics, fixed summation orders
    return out


def check(out, Theta, cnt, y, a0, Cs, tag):
    Ar, Ar_std, F, info, z = out
    s, r = Theta.shape
    n_p, q = len(y), Cs[0].shape[1]
    assert Ar.shape == (n_p, r) and Ar_std.shape == (n_p, r) and F.shape == (n_p, r, q) and info.shape == (n_p, 4)
    assert z.shape == (n_p, q) and np.all(info[:, 0] == 0)
    worst = 0.0
    for p in range(n_p):
        fid = y[p, :, 2].astype(int)
        y0, sig0 = (y[p, :, 0] - cnt) / SCALE[fid], y[p, :, 1] / SCALE[fid]
        ref = kalman_oracle(Theta, y0, sig0, a0[p], Cs[p])
        assert ref['kappa'] <= 1e8
        w = check_vector(ref, s, q, z=z[p], F=F[p], chi2=info[p, 2], logdet=info[p, 3])
        m = bar_factor(s, q, ref['kappa'])
        a_bar = m * float(np.linalg.norm(ref['z'])) * np.linalg.norm(Cs[p], 2) + 2 * EPS * np.linalg.norm(Ar[p])
        w = max(w, float(np.linalg.norm(Ar[p] - ref['a'])) / a_bar)
        cov = F[p].astype(LD) @ F[p].astype(LD).T
        sd = np.sqrt(np.diag(cov).astype(np.float64))
        assert np.all(np.abs(Ar_std[p] - sd) <= 4 * (q + 2) * EPS * sd), tag      # = sqrt(diag(F F^T)), q + 1 roundings
        assert 1.0 <= info[p, 1] <= ref['kappa'] * (1 + 1e-10)    # the pivots' ratio never exceeds cond_2(H')
        pinned = ~np.any(Cs[p] != 0, axis=1)
        assert np.array_equal(Ar[p][pinned], a0[p][pinned]) and not Ar_std[p][pinned].any() and not F[p][pinned].any()
        worst = max(worst, w)
    print(f'assimilate {tag}: worst error / bar {worst:.3e}')
    assert worst <= 1.0, (tag, worst)
    return worst


@pytest.mark.parametrize('s', [1, 15, 16, 17, 31, 32, 33, 70])
def test_sensor_counts_diagonal_prior(eng, s):
    Theta, cnt, y, a0, prior, Cs = draw(s, 17, 3, seed=s)
    check(run(eng, Theta, cnt, y, a0, prior, True), Theta, cnt, y, a0, Cs, f'diag s={s} r=17 n_p=3')


@pytest.mark.parametrize('r', [1, 15, 16, 17, 31, 32, 33, 47, 48, 64, 79, 80, 127, 128])
def test_mode_counts_diagonal_prior(eng, r):
    n_p = 3 if r < 100 else 2
    Theta, cnt, y, a0, prior, Cs = draw(33, r, n_p, seed=100 + r)
    check(run(eng, Theta, cnt, y, a0, prior, True), Theta, cnt, y, a0, Cs, f'diag s=33 r={r} n_p={n_p}')


@pytest.mark.parametrize('s,r', [(5, 8), (64, 128)])
def test_fewer_sensors_than_modes(eng, s, r):
    Theta, cnt, y, a0, prior, Cs = draw(s, r, 2, seed=200 + r)
    check(run(eng, Theta, cnt, y, a0, prior, True), Theta, cnt, y, a0, Cs, f'diag s={s} < r={r}')
    q = r - 1
    Theta, cnt, y, a0, prior, Cs = draw(s, r, 2, q=q, seed=210 + r)
    check(run(eng, Theta, cnt, y, a0, prior, False), Theta, cnt, y, a0, Cs, f'factor s={s} < r={r} q={q}')


@pytest.mark.parametrize('n_p', [1, 3, 65])
def test_vector_counts(eng, n_p):
    Theta, cnt, y, a0, prior, Cs = draw(17, 16, n_p, seed=300 + n_p)
    check(run(eng, Theta, cnt, y, a0, prior, True), Theta, cnt, y, a0, Cs, f'diag s=17 r=16 n_p={n_p}')
    Theta, cnt, y, a0, prior, Cs = draw(17, 16, n_p, q=5, seed=310 + n_p)
    check(run(eng, Theta, cnt, y, a0, prior, False), Theta, cnt, y, a0, Cs, f'factor s=17 r=16 q=5 n_p={n_p}')


@pytest.mark.parametrize('r', [1, 6, 17, 33, 128])
def test_factor_prior_ranks(eng, r):
    for q in sorted({1, max(r - 1, 1), r}):
        Theta, cnt, y, a0, prior, Cs = draw(33, r, 2, q=q, seed=400 + 3 * r + q)
        check(run(eng, Theta, cnt, y, a0, prior, False), Theta, cnt, y, a0, Cs, f'factor s=33 r={r} q={q}')


def test_pinned_coefficients_keep_their_bits(eng):
    Theta, cnt, y, a0, prior, Cs = draw(20, 17, 3, seed=500, zero_rows=True)
    a0[0, 0] = -0.0                                           # a pinned -0.0 keeps its sign bit too
    out = run(eng, Theta, cnt, y, a0, prior, True)
    check(out, Theta, cnt, y, a0, Cs, 'diag with zero sigmas and an all-zero row')
    assert np.array_equal(out[0][2], a0[2]) and not out[1][2].any() and not out[2][2].any() and not out[4][2].any()
    assert np.signbit(out[0][0, 0])
    Theta, cnt, y, a0, prior, Cs = draw(20, 17, 2, q=4, seed=501, zero_rows=True)
    check(run(eng, Theta, cnt, y, a0, prior, False), Theta, cnt, y, a0, Cs, 'factor with zero rows')


def test_padded_views_of_theta_and_y(eng):
    s, r = 21, 18
    Theta, cnt, y, a0, prior, Cs = draw(s, r, 3, seed=600)
    tb = np.full((s, r + 5), 7.5)
    tb[:, 2:2 + r] = Theta
    yb = np.full((3, s + 2, 4), -3.25)
    yb[:, 1:1 + s, :3] = y
    Theta_d, y_d = eng.to_device(tb)[:, 2:2 + r], eng.to_device(yb)[:, 1:1 + s, :3]
    assert not Theta_d.is_contiguous() and not y_d.is_contiguous()
    plain = run(eng, Theta, cnt, y, a0, prior, True)
    view = run(eng, Theta, cnt, y, a0, prior, True, Theta_d=Theta_d, y_d=y_d)
    for a, b in zip(plain, view):
        assert np.array_equal(a, b)
    check(view, Theta, cnt, y, a0, Cs, 'padded views')


def test_two_batches_equal_one_batch(eng):
    """sensors 1..s1, then s1+1..s with the first posterior (Ar, factor) as the prior, equals all s at once"""
    s, s1, r = 37, 16, 20
    Theta, cnt, y, a0, prior, Cs = draw(s, r, 3, seed=700)
    one = run(eng, Theta, cnt, y, a0, prior, True)
    first = run(eng, Theta[:s1], cnt[:s1], np.ascontiguousarray(y[:, :s1]), a0, prior, True)
    second = run(eng, Theta[s1:], cnt[s1:], np.ascontiguousarray(y[:, s1:]), first[0], first[2], False)
    worst = 0.0
    for p in range(3):
        fid = y[p, :, 2].astype(int)
        ref = kalman_oracle(Theta, (y[p, :, 0] - cnt) / SCALE[fid], y[p, :, 1] / SCALE[fid], a0[p], Cs[p])
        m = 2 * bar_factor(s, r, ref['kappa'])               # two updates, each within the bar of its own exact result
        cov = second[2][p].astype(LD) @ second[2][p].astype(LD).T
        e_a = float(np.linalg.norm((second[0][p] - a0[p]) / prior[p] - ref['z'])) / (m * float(np.linalg.norm(ref['z'])))
        e_c = float(np.linalg.norm(cov - ref['cov'])) / (m * float(np.linalg.norm(ref['cov'])))
        e_x = abs(first[3][p, 2] + second[3][p, 2] - float(ref['chi2'])) / (m * ref['wres2'])
        e_l = abs(first[3][p, 3] + second[3][p, 3] - float(ref['logdet'])) / (m * (r + ref['logabs']))
        worst = max(worst, e_a, e_c, e_x, e_l)
    print(f'assimilate two batches s={s1}+{s - s1} r={r}: worst error / bar {worst:.3e}')
    assert worst <= 1.0
    assert np.max(np.abs(second[0] - one[0])) <= 1e-9 * np.max(np.abs(one[0]))


def test_gpr_prior_to_field_end_to_end(eng):
    """GPR.predict(to_host=False) -> assimilate(to_host=False) -> reconstruct / reconstruct_std(factor=) on a 999-row,
    12-snapshot field against NumPy: the oracle's posterior pushed through  x = X_scl (Ur a) + X_cnt  in float64.
    Bars: the coefficient bars above carried through the linear map, |x - x_ref|_i <= scl_i |u_i| (m |z_ref| max sigma +
    8 r eps |a|) + 4 eps |x_ref|_i, and for the variance scl_i^2 |u_i|^2 m |cov_ref|_F + 8 (r + q) eps var_i."""
    from openmeasure_amd.gpr import GPR
    from openmeasure_amd.sparse_sensing import SPR
    rng = np.random.default_rng(5)
    n_points, F, m, r, s = 333, 3, 12, 4, 7
    P = np.column_stack([np.linspace(1.0, 4.0, m), 300 + 50 * rng.random(m)])
    g = np.linspace(0, 1, n_points)
    X = np.concatenate([(f + 1) * (np.sin(np.outer(g, P[:, 0]) + f) + 0.01 * np.outer(g * g, P[:, 1])) + 10 * f for f in range(F)])
    X = X + 1e-3 * rng.standard_normal(X.shape)
    gpr = GPR(X, F, None, P, engine=eng)
    gpr.fit(select_modes='number', n_modes=r)
    gpr.train(max_iter=40, rel_error=0.0)
    P_star = np.array([[2.2, 320.0], [3.3, 341.0]])
    A, S = gpr.predict(P_star, to_host=False)
    assert A.is_cuda and S.is_cuda
    spr = SPR(X, F, None, engine=eng)
    spr.fit(basis=(gpr.Ur, gpr.Ar))
    rows = np.sort(rng.choice(n_points * F, size=s, replace=False))
    C = np.zeros((s, n_points * F))
    C[np.arange(s), rows] = 1.0
    spr.train(C)
    scl = np.asarray(spr.X_scl)[:, 0]
    truth = 0.5 * (X[:, 3] + X[:, 8])
    ys = [np.stack([truth[rows] + 0.02 * scl[rows] * rng.standard_normal(s), 0.02 * scl[rows], (rows // n_points).astype(float)],
                   axis=1) for _ in range(2)]
    Ar, Ar_std, Fd = spr.assimilate(ys, A, S, to_host=False)
    assert Ar.is_cuda and Fd.is_cuda and tuple(Fd.shape) == (2, r, r)
    Xd, Xstd = spr.reconstruct(Ar), spr.reconstruct_std(factor=Fd)
    assert Xd.shape == (n_points * F, 2) and Xstd.shape == (n_points * F, 2)
    assert np.array_equal(Xstd, spr.reconstruct_std(factor=spr.assimilate(ys, A, S)[2]))
    info = spr.assimilate_info_
    assert np.all(info['status'] == 0) and np.all(info['dof'] == s) and info['prior'] == 'sigma'
    A_h, S_h = eng.to_host(A).copy(), eng.to_host(S).copy()
    U, cnt_x, Theta = np.asarray(spr.Ur, dtype=np.float64), np.asarray(spr.X_cnt)[:, 0], np.asarray(spr.Theta)
    cnt = eng.to_host(spr._d['cnt'])
    un = np.linalg.norm(U, axis=1)
    worst = 0.0
    for p, y in enumerate(ys):
        ref = kalman_oracle(Theta, (y[:, 0] - cnt) / scl[rows], y[:, 1] / scl[rows], A_h[p], np.diag(S_h[p]))
        assert ref['kappa'] <= 1e8
        mfac = bar_factor(s, r, ref['kappa'])
        a_ref, cov_ref = ref['a'].astype(np.float64), ref['cov'].astype(np.float64)
        x_ref = scl * (U @ a_ref) + cnt_x
        bar_x = scl * un * (mfac * float(np.linalg.norm(ref['z'])) * S_h[p].max() + 8 * r * EPS * np.linalg.norm(a_ref)) \
            + 4 * EPS * np.abs(x_ref)
        var_ref = scl ** 2 * np.einsum('ic,cd,id->i', U, cov_ref, U)
        bar_v = scl ** 2 * un ** 2 * mfac * np.linalg.norm(cov_ref) + 16 * r * EPS * var_ref
        worst = max(worst, np.max(np.abs(Xd[:, p] - x_ref) / bar_x), np.max(np.abs(Xstd[:, p] ** 2 - var_ref) / bar_v))
        assert abs(info['chi2'][p] - float(ref['chi2'])) <= mfac * ref['wres2']
    print(f'assimilate end to end (999 rows, r={r}, s={s}): worst error / bar {worst:.3e}')
    assert worst <= 1.0
