"""ROM.partial_fit on the HIP engine: the two kernels of csrc/update.hip against their longdouble restatements, and the
method against the SVD of everything seen, against the restated algorithm, sliced, inside the span, on f32 storage, into the
downstream chain, and refused.

The bars of the kernels are derived in tests/test_partial_fit_host.py (module docstring), whose functions compute them.  The
bars of the method are 100 x what the NumPy restatement of that file attains on the same input (the centre and scale the
object itself holds), at least 1e-13: the margin covers the different summation order of the device products.

Shapes of the kernel tests: n_points = 67, F = 3 (201 rows, both feature edges inside 64-row panels) with every r of
{1, 16, 17, 64, 65, 128} against every k of {1, 15, 16, 17, 64}; 1, 63, 64, 65 rows (one panel, full, one row over) and 4 099
rows (65 workgroups: the slot reduce matters) at the corners of that table; f32-stored X on the diagonal; leading dimensions
wider than the matrices (odd: the 8-byte loads; even: the 16-byte loads)."""
import pickle

import numpy as np
import pytest

from tests.test_partial_fit_host import (EXACT_BATCHES, EXACT_INIT, attained, bars_from, check_residual, exact_matrix,
                                         kernel_case, ld_basis_update, ld_residual, restate_init, restate_step, scaled,
                                         worst_ratio)

pytestmark = pytest.mark.gpu

RS = (1, 16, 17, 64, 65, 128)
KS = (1, 15, 16, 17, 64)
CORNERS = ((1, 1), (16, 16), (17, 15), (64, 64), (65, 17), (128, 64))
F32 = {(1, 1), (17, 15), (65, 17), (128, 64)}
# (n_points, F, r, k): 201 rows in three features; one feature of 1 / 63 / 64 / 65 / 4 099 rows
KERNEL_CASES = [(67, 3, r, k) for r in RS for k in KS] + [(n, 1, r, k) for n in (1, 63, 64, 65, 4099) for r, k in CORNERS]
PADS = ((0, 0), (1, 3), (2, 2))           # (ldu - r, ldx - k)


@pytest.fixture(scope='module')
def eng():
    from openmeasure_amd.engine import HipEngine
    return HipEngine('cuda:0')


def _dev(eng, A, pad=0, dtype=np.float64):
    """A as a column view of a device matrix `pad` columns wider"""
    import torch
    buf = np.zeros((A.shape[0], A.shape[1] + pad), dtype=dtype)
    buf[:, :A.shape[1]] = A
    t = eng.to_device(buf, dtype=torch.float32 if dtype == np.float32 else None)
    return t[:, :A.shape[1]]


def _case(eng, n_points, F, r, k, dtype, inside=False):
    i = (r + k + n_points) % len(PADS)
    c = kernel_case(n_points, F, r, k, seed=1000 + 7 * r + k + n_points, inside=inside, dtype=dtype)
    c['Ud'] = _dev(eng, c['U'], PADS[i][0])
    c['Xd'] = _dev(eng, c['X'], PADS[i][1], dtype)
    c['mu_d'], c['scale_d'] = eng.to_device(c['cnt']), eng.to_device(c['scale_f'])
    return c


def _residual(eng, c):
    H, C2, ss = eng.subspace_residual(c['Ud'], 0, c['n_points'], c['F'], c['mu_d'], c['scale_d'], c['Xd'],
                                      eng.to_device(c['C']))
    assert H._base is C2._base and H._base is ss._base
    return eng.to_host(H._base).copy()


def _check_residual(eng, c, tag):
    k, r = c['k'], c['r']
    out = _residual(eng, c)
    H, C2, ss = out[:k * k].reshape(k, k), out[k * k:k * k + k * r].reshape(k, r), out[-1:]
    assert np.array_equal(out, _residual(eng, c))                 # no atomics: two runs are bit-identical
    assert np.array_equal(H, H.T)                                 # H is bit-symmetric
    ref = ld_residual(c['U'], c['X'], c['cnt'], c['scale_f'], c['feat'], c['C'], c['F'])
    q = check_residual(H, C2, ss, ref)
    print('residual', tag, 'worst error / bar:', q)
    assert max(q.values()) <= 1.0, (tag, q)


@pytest.mark.parametrize('n_points,F,r,k', KERNEL_CASES, ids=[f'n{a * b}-r{r}-k{k}' for a, b, r, k in KERNEL_CASES])
def test_residual_kernel(eng, n_points, F, r, k):
    _check_residual(eng, _case(eng, n_points, F, r, k, np.float64), ('f64', n_points * F, r, k))
    if (r, k) in F32:
        _check_residual(eng, _case(eng, n_points, F, r, k, np.float32), ('f32', n_points * F, r, k))


@pytest.mark.parametrize('r,k', [(16, 16), (17, 15), (128, 64)])
def test_residual_kernel_batch_inside_the_span(eng, r, k):
    """E is rounding noise: H is held to its own bar (of the order u^2 |X0|^2), nothing relative to |X0|^2"""
    c = _case(eng, 67, 3, r, k, np.float64, inside=True)
    ref = ld_residual(c['U'], c['X'], c['cnt'], c['scale_f'], c['feat'], c['C'], c['F'])
    assert np.max(ref['bH']) < 1e-24 * float(ref['ss'])
    _check_residual(eng, c, ('inside', 201, r, k))


def _update(eng, c, A, B, r2, pad, sentinel=-7.25):
    import torch
    out = torch.full((c['n'], r2 + pad), sentinel, dtype=torch.float64, device=eng.device)
    res = eng.basis_update(c['Ud'], 0, c['n_points'], c['F'], c['mu_d'], c['scale_d'], c['Xd'] if B is not None else None,
                           eng.to_device(A), eng.to_device(B) if B is not None else None, out=out)
    assert res.data_ptr() == out.data_ptr()
    full = eng.to_host(out).copy()
    assert np.all(full[:, r2:] == sentinel)                       # columns beyond r2 are not written
    return full[:, :r2]


@pytest.mark.parametrize('n_points,F,r,k', KERNEL_CASES, ids=[f'n{a * b}-r{r}-k{k}' for a, b, r, k in KERNEL_CASES])
def test_basis_update_kernel(eng, n_points, F, r, k):
    rng = np.random.default_rng(r * 100 + k)
    for dtype in (np.float64, np.float32) if (r, k) in F32 else (np.float64,):
        c = _case(eng, n_points, F, r, k, dtype)
        # every output width at the corners, two of them (below and above r where there is one) elsewhere
        r2s = (1, 17, 64, 128) if (r, k) in CORNERS else ((1, 128) if r in (16, 17, 64) else (17, 64))
        for r2 in r2s:
            A, B = rng.standard_normal((r, r2)), rng.standard_normal((k, r2))
            pad = (r2 + k) % 3
            got = _update(eng, c, A, B, r2, pad)
            assert np.array_equal(got, _update(eng, c, A, B, r2, pad))      # two runs identical
            ref, bar = ld_basis_update(c['U'], c['X'], c['cnt'], c['scale_f'], c['feat'], A, B)
            q = worst_ratio(got, ref, bar)
            print('basis_update', dtype.__name__, n_points * F, r, k, r2, 'worst error / bar:', q)
            assert q <= 1.0
        A = rng.standard_normal((r, r2s[0]))                               # k = 0: a pure rotation
        got = _update(eng, c, A, None, r2s[0], 1)
        ref, bar = ld_basis_update(c['U'], None, c['cnt'], c['scale_f'], c['feat'], A, None)
        assert worst_ratio(got, ref, bar) <= 1.0


# ---------------------------------------------------------------------------------------------------- the method
def _spr(eng, X, F):
    from openmeasure_amd.sparse_sensing import SPR
    return SPR(X, F, None, engine=eng)


def _x0_of(rom, X):
    return (np.asarray(X, dtype=np.float64) - rom.X_cnt) / rom.X_scl


def _figures(rom, X0_all):
    """the device's figures, as tests.test_partial_fit_host.attained forms them for the restatement"""
    Uf, Sf, _ = np.linalg.svd(X0_all, full_matrices=False)
    U, S, r = rom.Ur, rom.Sigma_r, rom.r
    G = Uf[:, :r].T @ U
    seen = rom.Ar.shape[0]
    rec = rom.reconstruct(rom.Ar)                                  # (n, seen), physical units
    return dict(rec=float(np.max(np.abs(_x0_of(rom, rec) - X0_all[:, :seen])) / Sf[0]),
                S=float(np.max(np.abs(S - Sf[:r])) / Sf[0]),
                proj=float(np.linalg.norm(np.eye(r) - G @ G.T, 2)),
                orth=float(np.max(np.abs(U.T @ U - np.eye(r)))),
                expvar=float(abs(rom.exp_variance_[-1] - 100.0 * np.sum(Sf[:r] ** 2) / np.sum(Sf ** 2))))


def _exact(eng, X, F, tag):
    rom = _spr(eng, np.ascontiguousarray(X[:, :EXACT_INIT]), F)
    rom.fit(select_modes='number', n_modes=EXACT_INIT - 1)         # row centring: the 12-column block has rank 11
    X0 = _x0_of(rom, X)
    st = restate_init(X0[:, :EXACT_INIT], EXACT_INIT - 1)
    j = EXACT_INIT
    for kb in EXACT_BATCHES:
        rom.partial_fit(X[:, j:j + kb], select_modes='number', n_modes=rom.r + kb)
        st = restate_step(st, X0[:, j:j + kb])
        j += kb
        assert rom.r == st['S'].shape[0] and rom.n_seen_ == j and rom.Ar.shape == (j, rom.r)
        assert rom.Ur.shape == (X.shape[0], rom.r) and rom.Vr.shape == rom.Ar.shape
        assert rom.partial_fit_info_[-1]['q'] == kb
    bars, got = bars_from(attained(st, X0[:, :j])), _figures(rom, X0[:, :j])
    print('partial_fit exact', tag, 'device', got, 'bars', bars)
    for key in bars:
        assert got[key] <= bars[key], (key, got[key], bars[key])
    return rom


def test_method_equals_the_batch_svd(eng):
    X, n_points, F = exact_matrix()
    rom = _exact(eng, X, F, 'f64')
    assert rom.X.shape == (201, EXACT_INIT)                        # rom.X stays the initial block
    twin = pickle.loads(pickle.dumps(rom))                         # the new state pickles with the object
    assert twin.n_seen_ == 50 and twin._pf_E_tot == rom._pf_E_tot and twin.partial_fit_info_ == rom.partial_fit_info_
    assert np.array_equal(twin.Ar, rom.Ar) and np.array_equal(twin.exp_variance_, rom.exp_variance_)


def test_method_f32_storage(eng):
    """the snapshots stored as float32 (DeviceMatrix): the same assertions against the restatement fed the same f32 values"""
    import torch
    from openmeasure_amd.rom import DeviceMatrix
    X, n_points, F = exact_matrix()
    X32 = X.astype(np.float32)
    rom = _spr(eng, DeviceMatrix(eng.to_device(np.ascontiguousarray(X32[:, :EXACT_INIT]), dtype=torch.float32)), F)
    rom.fit(select_modes='number', n_modes=EXACT_INIT - 1)
    Xw = X32.astype(np.float64)
    X0 = _x0_of(rom, Xw)
    st = restate_init(X0[:, :EXACT_INIT], EXACT_INIT - 1)
    j = EXACT_INIT
    for kb in EXACT_BATCHES:
        batch = DeviceMatrix(eng.to_device(np.ascontiguousarray(X32[:, j:j + kb]), dtype=torch.float32))
        rom.partial_fit(batch, select_modes='number', n_modes=rom.r + kb)
        st = restate_step(st, X0[:, j:j + kb])
        j += kb
    bars, got = bars_from(attained(st, X0)), _figures(rom, X0)
    print('partial_fit exact f32 storage: device', got, 'bars', bars)
    for key in bars:
        assert got[key] <= bars[key], (key, got[key], bars[key])


def test_method_fixed_rank_equals_the_restatement(eng):
    """select_modes=None keeps r; S, the subspace and `dropped` are those of the restatement run with the same cap"""
    X, n_points, F = exact_matrix()
    r = 8
    rom = _spr(eng, np.ascontiguousarray(X[:, :EXACT_INIT]), F)
    rom.fit(select_modes='number', n_modes=r)
    X0 = _x0_of(rom, X)
    st = restate_init(X0[:, :EXACT_INIT], r)
    j = EXACT_INIT
    for kb in EXACT_BATCHES:
        rom.partial_fit(X[:, j:j + kb])
        st = restate_step(st, X0[:, j:j + kb], cap=r)
        j += kb
        assert rom.r == r and rom.Ur.shape == (201, r) and rom.Ar.shape == (j, r)
    stx, _x = restate_init(X0[:, :EXACT_INIT], EXACT_INIT - 1), EXACT_INIT
    for kb in EXACT_BATCHES:
        stx = restate_step(stx, X0[:, _x:_x + kb])
        _x += kb
    bars = bars_from(attained(stx, X0))
    G = st['U'].T @ rom.Ur
    got = dict(S=float(np.max(np.abs(rom.Sigma_r - st['S'])) / st['S'][0]), proj=float(np.linalg.norm(np.eye(r) - G @ G.T, 2)),
               orth=float(np.max(np.abs(rom.Ur.T @ rom.Ur - np.eye(r)))))
    print('partial_fit fixed rank: device against the restatement', got, 'bars', bars)
    for key in got:
        assert got[key] <= bars[key], (key, got[key], bars[key])
    for a, b in zip(rom.partial_fit_info_, st['info']):
        assert a['q'] == b['q']
        assert abs(a['dropped'] - b['dropped']) <= 2 * (r + 64) * bars['S'] * st['S'][0] ** 2, (a, b)
    assert np.all(np.diff(rom.exp_variance_) >= 0) and rom.exp_variance_[-1] <= 100.0 + 1e-9


def test_slices_of_64_are_full_updates(eng):
    """a batch of 64 + 9 columns equals the two calls, bit for bit"""
    X, n_points, F = exact_matrix(m=EXACT_INIT + 73)
    roms = []
    for split in (False, True):
        rom = _spr(eng, np.ascontiguousarray(X[:, :EXACT_INIT]), F)
        rom.fit(select_modes='number', n_modes=EXACT_INIT - 1)
        kw = dict(select_modes='number', n_modes=30)
        if split:
            rom.partial_fit(np.ascontiguousarray(X[:, EXACT_INIT:EXACT_INIT + 64]), **kw)
            rom.partial_fit(np.ascontiguousarray(X[:, EXACT_INIT + 64:]), **kw)
        else:
            rom.partial_fit(np.ascontiguousarray(X[:, EXACT_INIT:]), **kw)
        roms.append(rom)
    a, b = roms
    assert a.r == b.r == 30 and a.n_seen_ == b.n_seen_ == EXACT_INIT + 73 and len(a.partial_fit_info_) == 2
    assert np.array_equal(a.Ur, b.Ur) and np.array_equal(a.Ar, b.Ar) and np.array_equal(a.Sigma_r, b.Sigma_r)
    assert np.array_equal(a.exp_variance_, b.exp_variance_) and a.partial_fit_info_ == b.partial_fit_info_
    c = _spr(eng, np.ascontiguousarray(X[:, :EXACT_INIT]), F)
    c.fit(select_modes='number', n_modes=EXACT_INIT - 1)
    before = c._d['Ur']
    c.partial_fit(np.zeros((201, 0)))                              # no column: nothing happens
    assert c._d['Ur'] is before and 'n_seen_' not in c.__dict__


def test_a_deferred_projection_is_launched_first(eng):
    """fit() may only RECORD its projection (defer_project): partial_fit launches it and updates the basis it wrote -- the
    same bits as on an object that never defers"""
    rng = np.random.default_rng(4)
    X = rng.standard_normal((4224, 20)) @ rng.standard_normal((20, 64 + 16)) + 1e-3 * rng.standard_normal((4224, 80))
    roms = []
    for defer in (True, False):
        rom = _spr(eng, np.ascontiguousarray(X[:, :64]), 3)
        rom.defer_project = defer
        rom.fit(select_modes='number', n_modes=16)
        assert ('_proj_pending' in rom.__dict__) == defer
        rom.partial_fit(X[:, 64:], select_modes='number', n_modes=20)
        assert '_proj_pending' not in rom.__dict__ and rom.r == 20
        roms.append(rom)
    assert np.array_equal(roms[0].Ur, roms[1].Ur) and np.array_equal(roms[0].Ar, roms[1].Ar)


def test_batch_inside_the_span(eng):
    X, n_points, F = exact_matrix()
    rom = _spr(eng, np.ascontiguousarray(X[:, :EXACT_INIT]), F)
    rom.fit(select_modes='number', n_modes=EXACT_INIT - 1)
    X0 = _x0_of(rom, X[:, :EXACT_INIT])
    tol = 1e-7
    rom.partial_fit(np.ascontiguousarray(X[:, :5]), tol=tol)
    info = rom.partial_fit_info_[-1]
    assert info['q'] == 0 and rom.r == EXACT_INIT - 1 and rom.Ar.shape == (EXACT_INIT + 5, EXACT_INIT - 1)
    assert np.isfinite(info['orth_defect']) and info['residual'] < tol
    S_ref = np.linalg.svd(np.hstack([X0, X0[:, :5]]), compute_uv=False)[:rom.r]
    assert np.max(np.abs(rom.Sigma_r ** 2 - S_ref ** 2)) <= 1e-11 * S_ref[0] ** 2


def test_downstream_chain_runs_on_the_updated_fit(eng):
    from openmeasure_amd.sparse_sensing import SPR
    X, n_points, F = exact_matrix()
    Xi = np.ascontiguousarray(X[:, :EXACT_INIT])
    xt = X[:, 40]

    def y_fn(piv):
        y = np.zeros((len(piv), 3))
        y[:, 0] = xt[piv]
        y[:, 2] = piv // n_points
        return y

    def chain(spr):
        C = spr.optimal_placement()
        spr.train(C)
        a, _ = spr.predict(y_fn(spr.sensors_))
        return spr.sensors_.copy(), spr.reconstruct(a)

    rom = SPR(Xi, F, None, engine=eng)
    rom.fit(select_modes='number', n_modes=EXACT_INIT - 1)
    rom.train(rom.optimal_placement())
    assert 'Theta' in rom._d
    rom.partial_fit(X[:, 12:28], select_modes='number', n_modes=16)
    assert 'Theta' not in rom._d and 'Theta' not in rom.__dict__ and 'C' not in rom.__dict__     # trained before: gone
    s1, f1 = chain(rom)
    fresh = SPR(Xi, F, None, engine=eng)
    fresh.fit(basis=(rom.Ur, rom.Ar))
    s2, f2 = chain(fresh)
    assert np.array_equal(s1, s2)
    assert np.linalg.norm(f1 - f2) <= 1e-12 * np.linalg.norm(f2)
    A = rom.transform(X[:, 28:31])                                 # the other readers of the basis run
    assert A.shape == (3, 16) and np.all(np.isfinite(rom.reconstruction_error(X[:, 28:31])['rel_l2']))
    rom.fit(select_modes='number', n_modes=5)                      # a later fit() starts over from rom.X
    assert rom.r == 5 and rom.Ar.shape == (EXACT_INIT, 5) and 'n_seen_' not in rom.__dict__


def test_refusals_leave_the_fit_untouched(eng):
    import torch
    from openmeasure_amd._shard import RowShard
    from openmeasure_amd.gpr import GPR
    from openmeasure_amd.rom import DeviceMatrix
    from openmeasure_amd.sparse_sensing import SPR
    rng = np.random.default_rng(0)
    X = rng.standard_normal((201, 12 + 128))
    Xi = np.ascontiguousarray(X[:, :12])
    rom = SPR(Xi, 3, None, engine=eng)
    with pytest.raises(AttributeError):                            # not fitted: what transform raises
        rom.partial_fit(X[:, 12:20])
    rom.fit(select_modes='number', n_modes=11)
    rom.partial_fit(X[:, 12:76], select_modes='number', n_modes=200)
    assert rom.r == 75

    def frozen():
        return rom._d['Ur'], rom._d['Ur'].clone(), rom.Ar, rom.Ar.copy(), rom.r, len(rom.partial_fit_info_)

    def untouched(s):
        assert rom._d['Ur'] is s[0] and torch.equal(rom._d['Ur'], s[1]) and rom.Ar is s[2] and np.array_equal(rom.Ar, s[3])
        assert rom.r == s[4] and len(rom.partial_fit_info_) == s[5]

    s = frozen()
    with pytest.raises(NotImplementedError):                       # 75 + 64 modes > 128
        rom.partial_fit(X[:, 76:140], select_modes='number', n_modes=200)
    untouched(s)
    bad = X[:, 76:80].copy()
    bad[100, 2] = np.nan
    with pytest.raises(ValueError):
        rom.partial_fit(bad)
    untouched(s)
    bad[100, 2] = np.inf
    with pytest.raises(ValueError):
        rom.partial_fit(bad)
    untouched(s)
    with pytest.raises(ValueError):                                # a wrong row count
        rom.partial_fit(X[:200, 76:80])
    untouched(s)
    with pytest.raises(ValueError):
        rom.partial_fit(X[:, 76:80], select_modes='energy')
    untouched(s)
    # bases fit() did not compute in float64
    other = SPR(Xi, 3, None, engine=eng)
    other.fit(basis=(rom.Ur, rom.Ar))
    with pytest.raises(NotImplementedError, match='basis'):
        other.partial_fit(X[:, 76:80])
    other = SPR(Xi, 3, None, engine=eng)
    other.fit(select_modes='number', n_modes=11)
    other.Ur = other.Ur.copy()
    with pytest.raises(NotImplementedError, match='assigned'):
        other.partial_fit(X[:, 76:80])
    other = SPR(DeviceMatrix(eng.to_device(Xi.astype(np.float32), dtype=torch.float32), basis='f32'), 3, None, engine=eng)
    other.fit(select_modes='number', n_modes=11)
    with pytest.raises(NotImplementedError, match='float32'):
        other.partial_fit(X[:, 76:80])
    other = SPR(Xi, 3, None, shard=RowShard(0, 201), engine=eng)
    other.fit(select_modes='number', n_modes=11)
    with pytest.raises(NotImplementedError, match='sharded'):
        other.partial_fit(X[:, 76:80])
    with pytest.raises(NotImplementedError):
        GPR.partial_fit(GPR.__new__(GPR), X[:, 76:80])
