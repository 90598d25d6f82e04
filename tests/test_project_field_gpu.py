"""GPU tests (-m gpu) of the projection that emits the field (spr_project_field_*, csrc/project_ws.hip), of the row-dot
reconstruct kernel that shares its arithmetic (csrc/reconstruct.hip, csrc/field_dot.hpp) and of ROM.defer_project on the
HIP engine.

Shapes: F = 3, n_points = 1000 (no multiple of 16 or 128: every feature ends in a partial 16-row block and a partial
128-row chunk), (m, r) in {(64, 32), (128, 48), (256, 64)}, and n_points = 7 (fewer rows than one block).  The entry points
take any number of rows, so the KERNEL runs at all of these (test_kernel_*).  The host layer only records a projection
where the plain spr_project_* would take the same W-stationary kernel -- from 4096 rows on -- because only there do the two
routes store the same bits of Ur; at the shapes above a ROM therefore launches at once and the twin comparisons hold
trivially.  The same comparisons also run at n_points = 1500 (4500 rows: again no multiple of 16 or 128), where fit()
does defer and reconstruct() does fuse -- asserted, not assumed.

Tolerances.  Bitwise wherever two routes run the same arithmetic.  Against NumPy in float64: a dot product of K terms
accumulated in any order is within K eps sum|x_k y_k| of the exact one (eps = 2^-53 per rounding, K roundings at most per
term chain), and NumPy's own result within the same bound: 2 (K + 2) eps times the sum of absolute terms is asserted, entry
by entry.  Against the oracle: rel-Frobenius <= 1e-6, the bar of the golden fixtures (measured value printed)."""
import pickle

import numpy as np
import pytest

from oracle import spr_oracle as orc

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
ISSUE_SHAPES = [(1000, 3, 64, 32), (1000, 3, 128, 48), (1000, 3, 256, 64), (7, 3, 64, 32)]
FUSING_SHAPES = [(1500, 3, 64, 32), (1500, 3, 128, 48), (1500, 3, 256, 64)]


@pytest.fixture(scope='module')
def eng():
    from openmeasure_amd.engine import HipEngine
    return HipEngine()


def _snapshots(n_points, F, m, seed=5):
    """full-rank snapshots with a slowly decaying spectrum (sigma_64 / sigma_1 ~ 0.15: no refinement pass, no pre-centring)"""
    rng = np.random.default_rng(seed)
    n = n_points * F
    X = rng.standard_normal((n, m)) @ ((0.97 ** np.arange(m))[:, None] * rng.standard_normal((m, m))) / np.sqrt(m)
    for f in range(F):
        X[f * n_points:(f + 1) * n_points] = (f + 1) * X[f * n_points:(f + 1) * n_points] + 0.5 * f
    return np.ascontiguousarray(X)


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _field_call(eng, X, n_points, F, W, inv, mean, scale, A, basis32=False, norms=True):
    """spr_project_field_* called directly -> (Ur, nrm2 or None, field) as device tensors"""
    import torch
    from openmeasure_amd import _lib
    n, m = X.shape
    r = W.shape[1]
    f32 = X.dtype == torch.float32
    Ur = torch.full((n, r), float('nan'), dtype=torch.float32 if basis32 else torch.float64, device=X.device)
    nrm = torch.full((n,), float('nan'), dtype=torch.float64, device=X.device) if norms else None
    out = torch.full((A.shape[0], n), float('nan'), dtype=torch.float64, device=X.device)
    name = 'spr_project_field' + ('_f64' if not f32 else ('_x32' if basis32 else '_x32_f64out'))
    rc = getattr(eng.lib, name)(_ptr(X), n, m, X.stride(0), 0, n_points, F, _ptr(inv), _ptr(mean), _ptr(W), r, _ptr(Ur), r,
                                _ptr(nrm), _ptr(scale), _ptr(A), A.shape[0], _ptr(out), n, None)
    _lib.check(rc, name)
    return Ur, nrm, out


def _kernel_inputs(eng, n_points, F, m, r, f32=False):
    import torch
    rng = np.random.default_rng(11)
    n = n_points * F
    Xh = rng.standard_normal((n, m)) * 2.0 + 1.0
    if f32:
        Xh = Xh.astype(np.float32)
    X = eng.to_device(Xh, dtype=torch.float32 if f32 else None)
    Wh = rng.standard_normal((m, r)) / np.sqrt(m)
    inv_h, scale_h = 1.0 / (1.0 + np.arange(F)), 1.0 + np.arange(F) * 0.5
    mean_h = Xh.astype(np.float64).mean(axis=1)
    a_h = rng.standard_normal((1, r))
    dev = [eng.to_device(np.ascontiguousarray(v)) for v in (Wh, inv_h, mean_h, scale_h, a_h)]
    return (Xh, Wh, inv_h, mean_h, scale_h, a_h), (X, *dev)


@pytest.mark.parametrize('n_points,F,m,r', ISSUE_SHAPES + FUSING_SHAPES)
def test_kernel_against_numpy_and_standalone(eng, n_points, F, m, r):
    """The fused kernel at every shape: Ur, norms and field against float64 NumPy within the rounding bound of the sums,
    the field bit for bit against the stand-alone reconstruct on the Ur it stored, and -- where spr_project_norms_* takes the
    same kernel -- Ur and norms bit for bit against that entry point."""
    (Xh, Wh, inv_h, mean_h, scale_h, a_h), (X, W, inv, mean, scale, A) = _kernel_inputs(eng, n_points, F, m, r)
    Ur, nrm, field = _field_call(eng, X, n_points, F, W, inv, mean, scale, A)
    Ur_h, nrm_h, field_h = eng.to_host(Ur), eng.to_host(nrm), eng.to_host(field)
    assert np.all(np.isfinite(Ur_h)) and np.all(np.isfinite(nrm_h)) and np.all(np.isfinite(field_h))
    feat = np.arange(n_points * F) // n_points
    isc, sc = inv_h[feat][:, None], scale_h[feat]
    # Ur = (x W - mu 1^T W) / X_scl: m + 1 terms per entry, plus the column sum of W (m terms) and the scaling folded into W
    bound_u = 2 * (2 * m + 4) * EPS * ((np.abs(Xh) @ np.abs(Wh) + np.abs(mean_h)[:, None] * np.abs(Wh).sum(axis=0)) * isc)
    err_u = np.abs(Ur_h - ((Xh - mean_h[:, None]) @ Wh) * isc)
    print(f'Ur: max err / bound {np.max(err_u / bound_u):.3f}')
    assert np.all(err_u <= bound_u)
    sq = np.sum(Ur_h * Ur_h, axis=1)
    assert np.all(np.abs(nrm_h - sq) <= 2 * (r + 2) * EPS * sq)
    bound_f = 2 * (r + 2) * EPS * (sc * (np.abs(Ur_h) @ np.abs(a_h[0])) + np.abs(mean_h))
    err_f = np.abs(field_h[0] - (sc * (Ur_h @ a_h[0]) + mean_h))
    print(f'field: max err / bound {np.max(err_f / bound_f):.3f}')
    assert np.all(err_f <= bound_f)
    plain = eng.reconstruct(Ur, 0, n_points, F, mean, scale, A)
    assert np.array_equal(eng.to_host(plain), field_h)
    if eng.project_field_max(X, r):                                # the plain entry points take the same kernel here
        import torch
        nrm2 = torch.empty_like(nrm)
        Ur2 = eng.project(X, 0, n_points, F, inv, W, rowmean=mean, norms=nrm2)
        assert np.array_equal(eng.to_host(Ur2), Ur_h) and np.array_equal(eng.to_host(nrm2), nrm_h)
        Ur3, _, field3 = _field_call(eng, X, n_points, F, W, inv, mean, scale, A, norms=False)
        assert np.array_equal(eng.to_host(Ur3), Ur_h) and np.array_equal(eng.to_host(field3), field_h)
    else:
        assert n_points * F < 4096


@pytest.mark.parametrize('basis32', [True, False], ids=['f32-basis', 'f32-X-f64-basis'])
@pytest.mark.parametrize('n_points,F,m,r', [(1000, 3, 128, 48), (1500, 3, 256, 64)])
def test_kernel_f32_storage(eng, n_points, F, m, r, basis32):
    """f32 snapshots with an f32 or an f64 basis: the field comes from the values AS STORED, so it equals the stand-alone
    reconstruct on the stored basis bit for bit; the basis equals the plain projection's where that takes the same kernel."""
    import torch
    (Xh, Wh, inv_h, mean_h, scale_h, a_h), (X, W, inv, mean, scale, A) = _kernel_inputs(eng, n_points, F, m, r, f32=True)
    Ur, nrm, field = _field_call(eng, X, n_points, F, W, inv, mean, scale, A, basis32=basis32)
    assert Ur.dtype == (torch.float32 if basis32 else torch.float64)
    Ur_h, field_h = eng.to_host(Ur).astype(np.float64), eng.to_host(field)
    plain = eng.reconstruct(Ur, 0, n_points, F, mean, scale, A)
    assert np.array_equal(eng.to_host(plain), field_h)
    feat = np.arange(n_points * F) // n_points
    bound_f = 2 * (r + 2) * EPS * (scale_h[feat] * (np.abs(Ur_h) @ np.abs(a_h[0])) + np.abs(mean_h))
    assert np.all(np.abs(field_h[0] - (scale_h[feat] * (Ur_h @ a_h[0]) + mean_h)) <= bound_f)
    sq = np.sum(Ur_h * Ur_h, axis=1)
    assert np.all(np.abs(eng.to_host(nrm) - sq) <= 2 * (r + 2) * EPS * sq)
    if eng.project_field_max(X, r):
        Ur2 = eng.project(X, 0, n_points, F, inv, W, rowmean=mean, basis_dtype=Ur.dtype)
        assert np.array_equal(eng.to_host(Ur2), eng.to_host(Ur))


def _twins(eng, n_points, F, m, r, make=None):
    """-> (deferring object, twin with defer_project = False), both fitted on the same snapshots"""
    from openmeasure_amd.sparse_sensing import SPR
    X = _cached(('X', n_points, F, m), lambda: _snapshots(n_points, F, m))
    pair = []
    for defer in (True, False):
        s = SPR(make(X) if make else X, F, None, engine=eng)
        s.defer_project = defer
        s.fit(select_modes='number', n_modes=r)
        pair.append(s)
    a, b = pair
    assert np.array_equal(a.Ar, b.Ar) and '_proj_pending' not in b.__dict__
    fuses = eng.project_field_max(a._Xd(), r) > 0
    assert ('_proj_pending' in a.__dict__) == fuses
    assert fuses == (n_points * F >= 4096)
    return a, b, fuses


def _same_state(a, b, eng):
    assert '_proj_pending' not in a.__dict__
    assert np.array_equal(eng.to_host(a._d['Ur']), eng.to_host(b._d['Ur']))
    na, nb = a._d.get('nrm0'), b._d.get('nrm0')
    assert (na is None) == (nb is None)
    if na is not None:
        assert np.array_equal(eng.to_host(na), eng.to_host(nb))


@pytest.mark.parametrize('n_points,F,m,r', ISSUE_SHAPES + FUSING_SHAPES)
def test_fused_against_plain_and_twin(eng, n_points, F, m, r):
    a, b, fuses = _twins(eng, n_points, F, m, r)
    coef = b.Ar[0].copy()
    f1 = a.reconstruct(coef)                                   # fused where fit() deferred
    assert '_proj_pending' not in a.__dict__
    f2 = a.reconstruct(coef)                                   # stand-alone kernel on the basis the first call stored
    fb = b.reconstruct(coef)
    assert f1.shape == (n_points * F, 1)
    assert np.array_equal(f1, f2) and np.array_equal(f1, fb)
    _same_state(a, b, eng)
    # the device forms: same bits, same shapes, a PendingField for wait=False
    a.fit(select_modes='number', n_modes=r)
    d1 = a.reconstruct(eng.to_device(coef[None, :]), to_host=False)
    assert tuple(d1.shape) == (1, n_points * F) and np.array_equal(eng.to_host(d1)[0], fb[:, 0])
    a.fit(select_modes='number', n_modes=r)
    p1 = a.reconstruct(coef, to_host=False, wait=False)
    assert hasattr(p1, 'wait') and np.array_equal(eng.to_host(p1.wait())[0], fb[:, 0])
    _same_state(a, b, eng)


@pytest.mark.parametrize('how', ['Ur', 'optimal_placement', 'transform', 'pickle', 'second_fit', 'n_p_over', 'sampling'])
@pytest.mark.parametrize('n_points,F,m,r', [(1000, 3, 128, 48), (1500, 3, 128, 48)])
def test_flush_paths(eng, n_points, F, m, r, how):
    """Everything but a small reconstruct() launches the plain projection first (or, a second fit(), discards it): the
    twin's results, bit for bit."""
    import scipy.sparse as sp
    a, b, fuses = _twins(eng, n_points, F, m, r)
    n = n_points * F
    if how == 'Ur':
        assert np.array_equal(a.Ur, b.Ur)
    elif how == 'optimal_placement':
        Ca, Cb = a.optimal_placement(), b.optimal_placement()
        assert np.array_equal(a.sensors_, b.sensors_) and np.array_equal(np.asarray(Ca), np.asarray(Cb))
    elif how == 'transform':
        Xn = _cached(('X', n_points, F, m), None)[:, :3]
        assert np.array_equal(a.transform(Xn), b.transform(Xn))
    elif how == 'pickle':
        ca, cb = pickle.loads(pickle.dumps(a)), pickle.loads(pickle.dumps(b))
        assert np.array_equal(ca.Ur, cb.Ur)
    elif how == 'second_fit':
        a.fit(select_modes='number', n_modes=r)
        assert ('_proj_pending' in a.__dict__) == fuses
        assert np.array_equal(a.Ur, b.Ur)
    elif how == 'n_p_over':
        A = b.Ar[:eng.lib.spr_project_field_max() + 1].copy()
        assert np.array_equal(a.reconstruct(A), b.reconstruct(A))
    elif how == 'sampling':
        S = sp.csr_matrix((np.ones(5), (np.arange(5), np.array([0, 17, n_points, n - 1, n // 2]))), shape=(5, n))
        assert np.array_equal(a.reconstruct(b.Ar[0], sampling=S), b.reconstruct(b.Ar[0], sampling=S))
    if how != 'second_fit':
        assert '_proj_pending' not in a.__dict__
    _same_state(a, b, eng) if how != 'pickle' else None
    assert np.array_equal(a.reconstruct(b.Ar[0]), b.reconstruct(b.Ar[0]))


@pytest.mark.parametrize('basis', ['f32', None], ids=['f32-basis', 'f32-X-f64-basis'])
@pytest.mark.parametrize('n_points,F,m,r', [(1000, 3, 128, 48), (1500, 3, 128, 48)])
def test_storage_twins(eng, n_points, F, m, r, basis):
    import torch
    from openmeasure_amd.rom import DeviceMatrix
    a, b, fuses = _twins(eng, n_points, F, m, r,
                         make=lambda X: DeviceMatrix(eng.to_device(X.astype(np.float32), dtype=torch.float32), basis=basis))
    f1 = a.reconstruct(b.Ar[0])
    assert np.array_equal(f1, a.reconstruct(b.Ar[0])) and np.array_equal(f1, b.reconstruct(b.Ar[0]))
    assert a._d['Ur'].dtype == (torch.float32 if basis == 'f32' else torch.float64)
    _same_state(a, b, eng)


@pytest.mark.parametrize('n_points,F,m,r', ISSUE_SHAPES[:3] + FUSING_SHAPES)
def test_field_against_oracle(eng, n_points, F, m, r):
    a, _, _ = _twins(eng, n_points, F, m, r)
    X = _cached(('X', n_points, F, m), None)
    ref = _cached(('oracle', n_points, F, m, r), lambda: orc.fit(X, F, 'number', r))
    got = a.reconstruct(a.Ar[0])
    want = orc.reconstruct(ref['Ar'][0], ref['Ur'], ref['X_cnt'], ref['X_scl'])
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    print(f'field vs oracle ({n_points}, {F}, {m}, {r}): rel-Frobenius {err:.3e}')
    assert err <= 1e-6


def test_entry_point_argument_checks(eng):
    import torch
    n_points, F, m, r = 1000, 3, 64, 32
    _, (X, W, inv, mean, scale, A) = _kernel_inputs(eng, n_points, F, m, r)
    n = n_points * F
    lib = eng.lib
    nf = lib.spr_project_field_max()
    assert nf >= 1
    Ur = torch.empty((n, r), dtype=torch.float64, device=X.device)
    out = torch.zeros((nf + 1, n), dtype=torch.float64, device=X.device)
    A2 = torch.zeros((nf + 1, r), dtype=torch.float64, device=X.device)

    def call(**over):
        v = dict(X=_ptr(X), n=n, m=m, ldx=m, inv=_ptr(inv), mean=_ptr(mean), W=_ptr(W), r=r, Ur=_ptr(Ur), ldu=r, nrm=None,
                 scale=_ptr(scale), A=_ptr(A2), n_p=1, out=_ptr(out), ldo=n)
        v.update(over)
        return lib.spr_project_field_f64(v['X'], v['n'], v['m'], v['ldx'], 0, n_points, F, v['inv'], v['mean'], v['W'], v['r'],
                                         v['Ur'], v['ldu'], v['nrm'], v['scale'], v['A'], v['n_p'], v['out'], v['ldo'], None)
    for k in ('X', 'inv', 'mean', 'W', 'Ur', 'scale', 'A', 'out'):
        assert call(**{k: None}) == -1 and b'NULL' in lib.spr_last_error(), k
    assert call(n_p=0) == -1
    assert call(ldo=n - 1) == -1
    assert call(ldu=r - 1) == -1 and call(ldx=m - 1) == -1
    assert call(n_p=nf + 1) == -2 and b'n_p' in lib.spr_last_error()
    assert call(r=24, ldu=24) == -2                          # no whole 16-column tiles
    assert call(m=60, ldx=60) == -2                          # outside the W-stationary form
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0                     # nothing was launched by any refused call
    assert call() == 0                                       # ... and the same arguments, valid, run
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[0]).all()) and float(out[0].abs().sum()) > 0.0
