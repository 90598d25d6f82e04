"""ROM.partial_fit without a GPU: the algorithm, the host algebra of openmeasure_amd/_update.py, the bars the two kernels of
csrc/update.hip are held to, and the refusals of their launchers.

The algorithm is restated here in NumPy with every n-sized matrix explicit (``restate_step``): the new basis is formed as
[U, Q] P with Q the orthonormalised residual, NOT as U A + X0_b B, so the small matrices A and B that _update.py hands to
the basis-update kernel are checked against a different route.  The kernels' arithmetic is restated in np.longdouble
(``ld_residual``, ``ld_basis_update``); tests/test_partial_fit_gpu.py compares the device against them.

Bars (u = 2^-53; entrywise; T = the sum of the absolute values of the terms of the entry).  One v_mfma_f64_16x16x4_f64 step
adds four products to the accumulator, so a sum of L terms is a chain of ceil(L / 4) steps; the project's form is
(ceil(L / 4) + c) u T with c = 4 for the roundings outside the chain:
  * X0 = ((x - cnt) / scl): two roundings per element, 2 u |x0|, inside c wherever x0 is a factor.
  * E = X0 - U C^T, the accumulator starting at x0 and ceil(r / 4) steps:
        dE[i][j] = (ceil(r / 4) + 4) u (|x0[i][j]| + sum_c |U[i][c]| |C[j][c]|)
  * H = E^T E and C2 = E^T U: the rows of a workgroup's panels run through one accumulator, ceil(n / 4) steps at most, and
    the slots are added one after the other (at most ceil(n / 64) + F of them): D = ceil(n / 4) + ceil(n / 64) + F + 4, and
    with Ea = |E| + dE (what the device may hold in place of E)
        bar H[a][b]  = D u sum_i Ea[i][a] Ea[i][b] + sum_i (dE[i][a] |E[i][b]| + |E[i][a]| dE[i][b] + dE[i][a] dE[i][b])
        bar C2[j][c] = D u sum_i Ea[i][j] |U[i][c]| + sum_i dE[i][j] |U[i][c]|
    The error of E is propagated, second-order term included: for a batch inside span(U) E is rounding noise and the
    second-order term is what is left, so H is held to a bar of the order u^2 |X0|^2, nothing relative to |X0|^2.
  * ss = sum X0^2 in whatever order (per thread, per workgroup, per slot): (n k + 8) u ss, the bound of ANY order.
  * U_new = U A + X0 B: (ceil(r / 4) + ceil(k / 4) + 4) u (sum_c |U[i][c]| |A[c][j]| + sum_l |x0[i][l]| |B[l][j]|).

Attained by the restatement on the cases below (recorded by the tests that print them, float64 NumPy on the CPU):
  exact case (201 x 50, batches 12 | 5, 16, 17, nothing truncated, 49 modes down to 1e-3 of the first): |S - S_ref| / S_ref[0]
  3.3e-15, projector 8.3e-14, max |U^T U - I| 2.4e-14, exp_variance_[-1] 2.4e-13, reconstruction of the 50 snapshots 1e-15;
  capped case (rank-200 data, 264 snapshots, kept at 32 modes): error 0.2741 against the optimal 0.2719 (factor 1.008);
  ten batches of 16 at tol = 1e-7, spectrum over six decades, noise 1e-7: max |U^T U - I| 1.2e-3 without the C2 correction,
  2.1e-12 with it."""
import numpy as np
import pytest

from openmeasure_amd import _lib, _update

LD = np.longdouble
U53 = 2.0 ** -53


# ---------------------------------------------------------------------------------------------------- data and scaling
def exact_matrix(seed=7, n_points=67, F=3, m=50):
    """seeded (n_points F) x m matrix, singular values within three decades (nothing near tol), features of different
    offset and spread so that the frozen centre and the per-feature scale matter"""
    rng = np.random.default_rng(seed)
    n = n_points * F
    Q1, _ = np.linalg.qr(rng.standard_normal((n, m)))
    Q2, _ = np.linalg.qr(rng.standard_normal((m, m)))
    X = (Q1 * np.logspace(0, -3, m)) @ Q2.T * 40.0
    for f in range(F):
        X[f * n_points:(f + 1) * n_points] = (f + 1.5) * X[f * n_points:(f + 1) * n_points] + 3.0 * f - 2.0
    return X, n_points, F


def frozen_scaling(X_init, n_points, F):
    """centre (row means) and per-row scale (population std of the centred feature block) of the initial block"""
    cnt = X_init.mean(axis=1)
    Xc = X_init - cnt[:, None]
    scl = np.concatenate([np.full(n_points, Xc[f * n_points:(f + 1) * n_points].std()) for f in range(F)])
    return cnt, scl


def scaled(X, cnt, scl):
    return (X - cnt[:, None]) / scl[:, None]


# ---------------------------------------------------------------------------------------------------- the algorithm, restated
def restate_init(X0, r):
    U, S, Vt = np.linalg.svd(X0, full_matrices=False)
    return dict(U=U[:, :r].copy(), S=S[:r].copy(), V=Vt[:r].T.copy(), E_tot=float(np.sum(S ** 2)), info=[])


def restate_step(st, X0b, tol=1e-7, cap=None, correct=True):
    """one update with every n-sized matrix explicit; ``cap``: None = everything found, an int = at most that many modes"""
    U, S, V = st['U'], st['S'], st['V']
    r, k = S.shape[0], X0b.shape[1]
    C = X0b.T @ U
    E = X0b - U @ C.T
    H, C2, ss = E.T @ E, E.T @ U, float(np.sum(X0b * X0b))
    if correct:                                   # second pass of classical Gram-Schmidt
        E = E - U @ C2.T
        Ct, Hc = C + C2, H - C2 @ C2.T
    else:
        Ct, Hc = C, H
    Hc = (Hc + Hc.T) / 2
    lam, W = np.linalg.eigh(Hc)
    lam, W = lam[::-1], W[:, ::-1]
    q = int(np.sum(lam > (tol * max(S[0], np.sqrt(max(lam[0], 0.0)))) ** 2))
    T = W[:, :q] / np.sqrt(lam[:q])
    Q = E @ T                                     # (n, q), orthonormal, orthogonal to U
    K = np.block([[np.diag(S), Ct.T], [np.zeros((q, r)), T.T @ Hc]])
    P, sig, Wt = np.linalg.svd(K, full_matrices=False)
    r2 = r + q if cap is None else min(cap, r + q)
    Vbig = np.block([[V, np.zeros((V.shape[0], k))], [np.zeros((k, r)), np.eye(k)]])
    E_tot = st['E_tot'] + ss
    info = dict(q=q, dropped=float(np.sum(np.maximum(lam[q:], 0)) + np.sum(sig[r2:] ** 2)),
                residual=float(np.sqrt(max(np.trace(Hc), 0.0) / ss)), orth_defect=float(np.linalg.norm(C2) / np.sqrt(np.trace(H))))
    return dict(U=np.hstack([U, Q]) @ P[:, :r2], S=sig[:r2].copy(), V=Vbig @ Wt.T[:, :r2], E_tot=E_tot,
                info=st['info'] + [info], last=dict(C=C, H=H, C2=C2, ss=ss))


def attained(st, X0_all):
    """the four figures of the exact case against the SVD of everything seen"""
    Uf, Sf, _ = np.linalg.svd(X0_all, full_matrices=False)
    r = st['S'].shape[0]
    G = Uf[:, :r].T @ st['U']
    seen = st['V'].shape[0]
    return dict(rec=float(np.max(np.abs(st['U'] @ (st['V'] * st['S']).T - X0_all[:, :seen])) / Sf[0]),
                S=float(np.max(np.abs(st['S'] - Sf[:r])) / Sf[0]),
                proj=float(np.linalg.norm(np.eye(r) - G @ G.T, 2)),
                orth=float(np.max(np.abs(st['U'].T @ st['U'] - np.eye(r)))),
                expvar=float(abs(100.0 * np.sum(st['S'] ** 2) / st['E_tot'] - 100.0 * np.sum(Sf[:r] ** 2) / np.sum(Sf ** 2))))


EXACT_BATCHES = (5, 16, 17)
EXACT_INIT = 12


def exact_case_restated():
    """-> (restated state after the three batches, X0 of all 50 columns, cnt, scl, X, n_points, F)"""
    X, n_points, F = exact_matrix()
    cnt, scl = frozen_scaling(X[:, :EXACT_INIT], n_points, F)
    X0 = scaled(X, cnt, scl)
    st = restate_init(X0[:, :EXACT_INIT], EXACT_INIT - 1)          # row centring: the 12-column block has rank 11
    j = EXACT_INIT
    for kb in EXACT_BATCHES:
        st = restate_step(st, X0[:, j:j + kb])
        j += kb
    return st, X0, cnt, scl, X, n_points, F


def bars_from(att, floor=1e-13, margin=100.0):
    """the device bars: 100 x what the restatement attains, at least 1e-13 (the margin covers another summation order)"""
    return {k: max(margin * v, floor) for k, v in att.items()}


def test_restatement_equals_the_batch_svd():
    st, X0, *_ = exact_case_restated()
    att = attained(st, X0)
    print('exact case, restatement attains:', att)
    assert st['S'].shape[0] == EXACT_INIT - 1 + sum(EXACT_BATCHES) == 49
    assert att['S'] < 1e-13 and att['proj'] < 1e-11 and att['orth'] < 1e-12 and att['expvar'] < 1e-11
    assert st['V'].shape[0] == 50 and att['rec'] < 1e-12         # Ar = V diag(S) reconstructs every snapshot seen


def capped_case(cap=32, seed=11):
    rng = np.random.default_rng(seed)
    n, m = 900, 264
    Q1, _ = np.linalg.qr(rng.standard_normal((n, 200)))
    X0 = (Q1 * (1.0 / (1.0 + np.arange(200)) ** 0.75)) @ rng.standard_normal((200, m)) / np.sqrt(m)
    st = restate_init(X0[:, :40], cap)
    for j in range(40, m, 32):
        st = restate_step(st, X0[:, j:j + 32], cap=cap)
    return st, X0


def test_capped_update_is_close_to_optimal_not_equal():
    st, X0 = capped_case()
    S = np.linalg.svd(X0, compute_uv=False)
    opt = np.sqrt(np.sum(S[32:] ** 2) / np.sum(S ** 2))
    err = np.linalg.norm(X0 - st['U'] @ (st['U'].T @ X0)) / np.linalg.norm(X0)
    print('capped case: error', err, 'optimal', opt, 'factor', err / opt)
    assert opt <= err * (1 + 1e-12)
    assert err <= 1.05 * opt                        # the restatement attains 1.008 (docstring); truncation loses a little


def many_batches(correct, tol=1e-7, seed=3):
    rng = np.random.default_rng(seed)
    n, m = 1500, 176
    Q1, _ = np.linalg.qr(rng.standard_normal((n, 60)))
    X0 = (Q1 * np.logspace(0, -6, 60)) @ rng.standard_normal((60, m)) + 1e-7 * rng.standard_normal((n, m))
    st = restate_init(X0[:, :16], 16)
    for j in range(16, m, 16):
        st = restate_step(st, X0[:, j:j + 16], tol=tol, correct=correct)
    r = st['S'].shape[0]
    return float(np.max(np.abs(st['U'].T @ st['U'] - np.eye(r))))


def test_the_c2_correction_is_required():
    """why the residual kernel returns C2: without it the orthogonality lost in U A + X0 B re-enters the next residual"""
    without, with_ = many_batches(False), many_batches(True)
    print('ten batches of 16, tol 1e-7: max |U^T U - I| without C2', without, 'with', with_)
    assert with_ < 1e-8
    assert without > 1e4 * with_


# ---------------------------------------------------------------------------------------------------- _update.py against the restatement
def _host_function_follows(st0, batches, **kw):
    st = st0
    S, Ar, E_tot, U = st['S'], st['V'] * st['S'], st['E_tot'], st['U']
    for X0b in batches:
        st = restate_step(st, X0b, tol=kw.get('tol', 1e-7), cap=kw.get('cap'))
        la = st['last']
        sel = dict(select_modes='number', n_modes=10 ** 6) if kw.get('cap') is None else \
            dict(select_modes='number', n_modes=kw['cap'])
        up = _update.svd_update(S, Ar, la['C'], la['H'], la['C2'], la['ss'], E_tot, tol=kw.get('tol', 1e-7), **sel)
        U = U @ up['A'] + X0b @ up['B']
        S, Ar, E_tot = up['S'], up['Ar'], up['E_tot']
        sgn = np.sign(np.sum(U * st['U'], axis=0))                  # the SVD's signs are LAPACK's in both
        assert np.max(np.abs(S - st['S'])) <= 1e-13 * st['S'][0]
        assert np.max(np.abs(U * sgn - st['U'])) <= 1e-13 * max(1.0, st['S'][0] / st['S'][-1])
        assert np.max(np.abs(Ar * sgn - st['V'] * st['S'])) <= 1e-13 * st['S'][0] * max(1.0, st['S'][0] / st['S'][-1])
        assert abs(E_tot - st['E_tot']) <= 1e-13 * E_tot
        for key in ('q', 'dropped', 'residual', 'orth_defect'):
            a, b = up[key], st['info'][-1][key]
            assert a == b or abs(a - b) <= 1e-10 * max(abs(a), abs(b)) + 1e-13 * st['S'][0] ** 2, (key, a, b)
        # the restatement continues from ITS state; the host function from its own: they are compared every step
    return st


def test_host_function_equals_the_restatement_exact():
    X, n_points, F = exact_matrix()
    cnt, scl = frozen_scaling(X[:, :EXACT_INIT], n_points, F)
    X0 = scaled(X, cnt, scl)
    cuts = np.cumsum((EXACT_INIT,) + EXACT_BATCHES)
    _host_function_follows(restate_init(X0[:, :EXACT_INIT], EXACT_INIT - 1),
                           [X0[:, a:b] for a, b in zip(cuts[:-1], cuts[1:])])


def test_host_function_equals_the_restatement_capped():
    rng = np.random.default_rng(5)
    X0 = rng.standard_normal((300, 20)) @ rng.standard_normal((20, 60)) + 1e-3 * rng.standard_normal((300, 60))
    _host_function_follows(restate_init(X0[:, :12], 8), [X0[:, 12:28], X0[:, 28:60]], cap=8)


def test_host_function_rank_rules_and_refusals():
    st, X0, *_ = exact_case_restated()
    st0 = restate_init(X0[:, :12], 11)
    la = restate_step(st0, X0[:, 12:17])['last']
    args = (st0['S'], st0['V'] * st0['S'], la['C'], la['H'], la['C2'], la['ss'], st0['E_tot'])
    assert _update.svd_update(*args)['S'].shape == (11,)                                  # None keeps r
    assert _update.svd_update(*args, select_modes='number', n_modes=13)['S'].shape == (13,)
    assert _update.svd_update(*args, select_modes='number', n_modes=99)['S'].shape == (16,)   # at most r + q
    up = _update.svd_update(*args, select_modes='variance', n_modes=90.0)
    assert up['exp_variance'][-1] >= 90.0 and (len(up['S']) == 1 or up['exp_variance'][-2] < 90.0)
    with pytest.raises(NotImplementedError):
        _update.svd_update(*args, select_modes='number', n_modes=16, max_rank=15)
    bad = la['H'].copy()
    bad[0, 0] = np.nan
    with pytest.raises(ValueError):
        _update.svd_update(args[0], args[1], la['C'], bad, la['C2'], la['ss'], st0['E_tot'])
    with pytest.raises(ValueError):
        _update.svd_update(args[0], args[1], la['C'], la['H'], la['C2'], np.inf, st0['E_tot'])
    assert abs(_update.initial_energy(st0['S'], 100 * np.cumsum(st0['S'] ** 2) / st0['E_tot']) - st0['E_tot']) < 1e-12 * st0['E_tot']


# ---------------------------------------------------------------------------------------------------- the kernels' arithmetic in longdouble
def feature_of_rows(n, row0, n_points, F):
    return np.minimum((row0 + np.arange(n)) // n_points, F - 1)


def ld_x0(X, cnt, scale_f, feat):
    return (X.astype(LD) - cnt.astype(LD)[:, None]) / scale_f.astype(LD)[feat][:, None]


def ld_residual(U, X, cnt, scale_f, feat, C, F):
    """longdouble H, C2, ss of the residual kernel and their bars (module docstring) -> dict"""
    n, r = U.shape
    k = X.shape[1]
    Ul, Cl = U.astype(LD), C.astype(LD)
    x0 = ld_x0(X, cnt, scale_f, feat)
    E = x0 - Ul @ Cl.T
    aU, aE = np.abs(Ul), np.abs(E)
    dE = (np.ceil(r / 4) + 4) * U53 * (np.abs(x0) + aU @ np.abs(Cl).T)
    Ea = aE + dE
    D = (np.ceil(n / 4) + np.ceil(n / 64) + F + 4) * U53
    ss = np.sum(x0 * x0)
    return dict(H=E.T @ E, C2=E.T @ Ul, ss=ss,
                bH=D * (Ea.T @ Ea) + dE.T @ aE + aE.T @ dE + dE.T @ dE,
                bC2=D * (Ea.T @ aU) + dE.T @ aU, bss=(n * k + 8) * U53 * ss)


def ld_basis_update(U, X, cnt, scale_f, feat, A, B):
    """longdouble U A + X0 B and its bar -> (out, bar)"""
    r = U.shape[1]
    k = 0 if X is None else X.shape[1]
    Ul, Al = U.astype(LD), A.astype(LD)
    out, T = Ul @ Al, np.abs(Ul) @ np.abs(Al)
    if k:
        x0, Bl = ld_x0(X, cnt, scale_f, feat), B.astype(LD)
        out, T = out + x0 @ Bl, T + np.abs(x0) @ np.abs(Bl)
    return out, (np.ceil(r / 4) + np.ceil(k / 4) + 4) * U53 * T


def worst_ratio(got, ref, bar):
    """max |got - ref| / bar over the entries (an entry with bar 0 must be exact)"""
    err = np.abs(np.asarray(got).astype(LD) - ref)
    bar = np.asarray(bar, dtype=LD)
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(bar > 0, err / bar, np.where(err > 0, np.inf, 0.0))
    return float(np.max(q))


def check_residual(H, C2, ss, ref):
    """-> dict of worst error / bar per output; all <= 1 is a pass"""
    return dict(H=worst_ratio(H, ref['H'], ref['bH']), C2=worst_ratio(C2, ref['C2'], ref['bC2']),
                ss=worst_ratio(np.asarray(ss).reshape(-1)[:1], np.asarray([ref['ss']]), np.asarray([ref['bss']])))


def kernel_case(n_points, F, r, k, seed, inside=False, dtype=np.float64, row0=0, n=None):
    """a block of rows with a basis orthonormal to rounding, a batch, centre, per-feature scale and C = X0^T U (f64 NumPy);
    ``inside``: the batch lies in span(U) (E = rounding noise)"""
    rng = np.random.default_rng(seed)
    n = n_points * F - row0 if n is None else n
    U = np.linalg.qr(rng.standard_normal((n, r)))[0] if n >= r else rng.standard_normal((n, r)) / np.sqrt(r)
    feat = feature_of_rows(n, row0, n_points, F)
    cnt = rng.standard_normal(n) * 3.0
    scale_f = 0.5 + 2.0 * rng.random(F) * (1 + np.arange(F))
    if inside:
        x0 = U @ rng.standard_normal((r, k))
    else:
        x0 = U @ rng.standard_normal((r, k)) + 0.3 * rng.standard_normal((n, k))
    X = (x0 * scale_f[feat][:, None] + cnt[:, None]).astype(dtype)
    C = (((X.astype(np.float64) - cnt[:, None]) / scale_f[feat][:, None]).T @ U)
    return dict(U=U, X=X, cnt=cnt, scale_f=scale_f, feat=feat, C=C, n=n, r=r, k=k, F=F, n_points=n_points, row0=row0)


def np_residual(c, wrong=None):
    """float64 NumPy restatement of the residual kernel; ``wrong`` names one deliberate defect"""
    X = c['X'].astype(np.float64)
    feat = c['feat']
    if wrong == 'edge_scale':                    # the first row of feature 1 divided by the scale of feature 0
        feat = feat.copy()
        feat[np.flatnonzero(feat == 1)[0]] = 0
    x0 = (X - (0.0 if wrong == 'no_centre' else c['cnt'][:, None])) / c['scale_f'][feat][:, None]
    E = x0 if wrong == 'no_C' else x0 - c['U'] @ c['C'].T
    H = x0.T @ x0 - c['C'] @ c['C'].T if wrong == 'gram_difference' else E.T @ E
    return H, E.T @ c['U'], np.sum(x0 * x0)


@pytest.mark.parametrize('inside', [False, True])
def test_checker_accepts_the_float64_restatement(inside):
    c = kernel_case(67, 3, 17, 15, seed=21, inside=inside)
    ref = ld_residual(c['U'], c['X'], c['cnt'], c['scale_f'], c['feat'], c['C'], c['F'])
    q = check_residual(*np_residual(c), ref)
    print('float64 NumPy against the longdouble restatement, worst error / bar:', q)
    assert max(q.values()) <= 1.0


@pytest.mark.parametrize('wrong,inside,field', [('no_C', False, 'H'), ('no_centre', False, 'ss'),
                                                ('gram_difference', True, 'H'), ('edge_scale', False, 'ss')])
def test_checker_rejects_wrong_restatements(wrong, inside, field):
    c = kernel_case(67, 3, 17, 15, seed=22, inside=inside)
    ref = ld_residual(c['U'], c['X'], c['cnt'], c['scale_f'], c['feat'], c['C'], c['F'])
    q = check_residual(*np_residual(c, wrong), ref)
    assert q[field] > 1.0, (wrong, q)


def test_checker_for_the_basis_update():
    c = kernel_case(67, 3, 17, 15, seed=23)
    rng = np.random.default_rng(1)
    A, B = rng.standard_normal((17, 20)), rng.standard_normal((15, 20))
    ref, bar = ld_basis_update(c['U'], c['X'], c['cnt'], c['scale_f'], c['feat'], A, B)
    x0 = (c['X'] - c['cnt'][:, None]) / c['scale_f'][c['feat']][:, None]
    assert worst_ratio(c['U'] @ A + x0 @ B, ref, bar) <= 1.0
    assert worst_ratio(c['U'] @ A + c['X'] @ B, ref, bar) > 1.0            # centre and scale not applied
    feat = c['feat'].copy()
    feat[np.flatnonzero(feat == 2)[0]] = 1                                  # the neighbour's scale at a segment edge
    x0w = (c['X'] - c['cnt'][:, None]) / c['scale_f'][feat][:, None]
    assert worst_ratio(c['U'] @ A + x0w @ B, ref, bar) > 1.0
    assert worst_ratio(c['U'] @ A, *ld_basis_update(c['U'], None, c['cnt'], c['scale_f'], c['feat'], A, None)) <= 1.0


# ---------------------------------------------------------------------------------------------------- refusals of the launchers
INVALID, UNSUPPORTED = -1, -2
P = [8 * (i + 1) for i in range(12)]     # stand-in non-NULL pointers, never dereferenced: every call here is refused
BIG = 1 << 40

RESIDUAL = ('Ur n_rows r ldu X k ldx row0 n_points n_features rowmean scale C H C2 ss ws ws_bytes stream',
            dict(Ur=P[0], n_rows=100, r=8, ldu=8, X=P[1], k=3, ldx=3, row0=0, n_points=50, n_features=2, rowmean=P[2],
                 scale=P[3], C=P[4], H=P[5], C2=P[6], ss=P[7], ws=P[8], ws_bytes=BIG, stream=None))
UPDATE = ('Ur n_rows r ldu X k ldx row0 n_points n_features rowmean scale A B r2 out ldo stream',
          dict(Ur=P[0], n_rows=100, r=8, ldu=8, X=P[1], k=3, ldx=3, row0=0, n_points=50, n_features=2, rowmean=P[2],
               scale=P[3], A=P[4], B=P[5], r2=8, out=P[6], ldo=8, stream=None))
FAMILIES = {'spr_subspace_residual_f64': RESIDUAL, 'spr_subspace_residual_x32': RESIDUAL,
            'spr_basis_update_f64': UPDATE, 'spr_basis_update_x32': UPDATE}

# (family filter, changes to the well-formed set, status, words of the text): where two defects are present the first
# listed check fires -- pointers, shape, layout, r, k, then r2, ldo
REFUSALS = [
    ('', dict(Ur=None), INVALID, 'NULL pointer'),
    ('', dict(rowmean=None, r=129, ldu=129), INVALID, 'NULL pointer'),                  # pointers before r
    ('', dict(r=129, ldu=129), UNSUPPORTED, 'r = 129'),
    ('', dict(r=129, ldu=128), INVALID, 'bad shape'),                                  # shape before r
    ('', dict(k=65, ldx=65), UNSUPPORTED, 'k = 65'),
    ('', dict(r=129, ldu=129, k=65, ldx=65), UNSUPPORTED, 'r = 129'),                  # r before k
    ('', dict(k=-1), INVALID, 'bad shape'),
    ('', dict(n_points=49), INVALID, 'bad feature layout'),
    ('', dict(n_points=49, k=65, ldx=65), INVALID, 'bad feature layout'),              # layout before k
    ('residual', dict(k=0), INVALID, 'k = 0'),
    ('residual', dict(ws_bytes=8), INVALID, 'workspace'),
    ('residual', dict(C=None), INVALID, 'NULL pointer'),
    ('update', dict(r2=129, ldo=129), UNSUPPORTED, 'r2 = 129'),
    ('update', dict(r2=129, ldo=8), UNSUPPORTED, 'r2 = 129'),                          # r2 before ldo
    ('update', dict(r2=16, ldo=15), INVALID, 'ldo = 15'),
    ('update', dict(r2=0), INVALID, 'bad shape r2'),
    ('update', dict(k=65, ldx=65, r2=129, ldo=129), UNSUPPORTED, 'k = 65'),            # k before r2
    ('update', dict(out=P[0]), INVALID, 'over the old one'),
    ('update', dict(B=None), INVALID, 'NULL pointer'),
    ('update', dict(k=0, X=None, B=None, r2=129, ldo=129), UNSUPPORTED, 'r2 = 129'),   # k = 0 needs neither X nor B
]
CASES = [(name, i) for name in FAMILIES for i, rf in enumerate(REFUSALS) if rf[0] in name]


@pytest.mark.parametrize('name,i', CASES, ids=[f'{n}-{i}' for n, i in CASES])
def test_launcher_refusals(name, i):
    lib = _lib.load()
    order, good = FAMILIES[name]
    _, change, status, words = REFUSALS[i]
    args = dict(good, **change)
    rc = getattr(lib, name)(*[args[a] for a in order.split()])
    msg = lib.spr_last_error().decode()
    assert rc == status, (rc, msg)
    assert msg.startswith(name + ':') and words in msg, msg


def test_workspace_query_refuses_what_the_launcher_refuses():
    lib = _lib.load()
    assert lib.spr_subspace_residual_workspace(128, 64, 3) > 0
    for r, k, F in ((129, 64, 3), (128, 65, 3), (0, 1, 1), (8, 0, 1), (8, 8, 0)):
        assert lib.spr_subspace_residual_workspace(r, k, F) == 0
