"""GPU tests (-m gpu) of the edges of the W-stationary projection kernel (csrc/project_ws.hip): every LDS addressing form,
padded column tiles, partial chunks and partial 16-row blocks, shards that cut features, more chunks than workgroups, and
the four epilogue forms (with / without the row norms, with / without the field).

Row counts are the smallest at which spr_project_* / spr_project_norms_* still hand the shape to this kernel (4096 rows;
spr_project_field_* takes it at any row count):
  * m = 256, r = 64: the only shape whose LDS image of W passes 64 KB (the second base register);
  * m = 256, r = 48: a padded column tile (r < 16 RT);
  * m = 128, r = 32 and m = 192, r = 64: the two- and four-tile forms below 64 KB;
  all four with F = 3, n_points = 1371: 4113 rows, so every feature ends in a partial 128-row chunk and a partial 16-row
  block, and the feature boundaries fall inside 16-row blocks of the matrix;
  * a shard of rows [700, 5200) of a 3 x 2000 matrix: it starts and ends inside a feature;
  * F = 9, n_points = 5157: 41 chunks per feature, 369 in all -- more than one per workgroup.

References.  Ur, the norms and the field are compared entry by entry with a NumPy long-double evaluation, under the bars
tests/test_project_field_gpu.py uses for these quantities: a dot product of K terms in any order is within K eps sum|x_k y_k|
of the exact one (eps = 2^-53); 2 (K + 2) eps times the sum of absolute terms is asserted.  Every comparison between two
launches of the same arithmetic is bitwise."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
LD = np.longdouble

# (n_points, F, m, r, row0, n_rows); row0 / n_rows None: the whole matrix
SHAPES = [
    pytest.param(1371, 3, 256, 64, None, None, id='m256-r64'),
    pytest.param(1371, 3, 256, 48, None, None, id='m256-r48-padded-tile'),
    pytest.param(1371, 3, 128, 32, None, None, id='m128-r32'),
    pytest.param(1371, 3, 192, 64, None, None, id='m192-r64'),
    pytest.param(2000, 3, 256, 64, 700, 4500, id='shard-inside-features'),
    pytest.param(5157, 9, 128, 32, None, None, id='F9-369-chunks'),
]


@pytest.fixture(scope='module')
def eng():
    from openmeasure_amd.engine import HipEngine
    return HipEngine()


def _ptr(t):
    return t.data_ptr() if t is not None else None


_CACHE = {}


def _case(eng, n_points, F, m, r, row0, n_rows):
    """Inputs on host and device and the long-double reference of Ur, computed once per shape."""
    key = (n_points, F, m, r, row0, n_rows)
    if key in _CACHE:
        return _CACHE[key]
    row0 = 0 if row0 is None else row0
    n = n_points * F - row0 if n_rows is None else n_rows
    rng = np.random.default_rng(7 * m + r + n)
    Xh = rng.standard_normal((n, m)) * 2.0 + 1.0
    Wh = rng.standard_normal((m, r)) / np.sqrt(m)
    inv_h, scale_h = 1.0 / (1.0 + np.arange(F)), 1.0 + 0.5 * np.arange(F)
    mean_h = Xh.mean(axis=1)
    a_h = rng.standard_normal((1, r))
    feat = (row0 + np.arange(n)) // n_points
    Ur_ref = ((Xh.astype(LD) - mean_h.astype(LD)[:, None]) @ Wh.astype(LD)) * inv_h[feat].astype(LD)[:, None]
    # Ur = (x W - mu 1^T W) / X_scl: m + 1 terms per entry, plus the column sum of W (m terms) and the scaling folded into W
    bound_u = 2 * (2 * m + 4) * EPS * ((np.abs(Xh) @ np.abs(Wh) + np.abs(mean_h)[:, None] * np.abs(Wh).sum(axis=0))
                                       * inv_h[feat][:, None])
    host = dict(X=Xh, W=Wh, inv=inv_h, scale=scale_h, mean=mean_h, a=a_h, feat=feat, Ur_ref=Ur_ref, bound_u=bound_u,
                row0=row0, n=n)
    dev = {k: eng.to_device(np.ascontiguousarray(host[k])) for k in ('X', 'W', 'inv', 'mean', 'scale', 'a')}
    _CACHE[key] = (host, dev)
    return host, dev


def _field_call(eng, dev, row0, n_points, F, norms=True):
    """spr_project_field_f64 called directly -> (Ur, nrm2 or None, field) on the host; every output starts as NaN"""
    import torch
    from openmeasure_amd import _lib
    X, W, A = dev['X'], dev['W'], dev['a']
    n, m = X.shape
    r = W.shape[1]
    Ur = torch.full((n, r), float('nan'), dtype=torch.float64, device=X.device)
    nrm = torch.full((n,), float('nan'), dtype=torch.float64, device=X.device) if norms else None
    out = torch.full((A.shape[0], n), float('nan'), dtype=torch.float64, device=X.device)
    rc = eng.lib.spr_project_field_f64(_ptr(X), n, m, X.stride(0), row0, n_points, F, _ptr(dev['inv']), _ptr(dev['mean']),
                                       _ptr(W), r, _ptr(Ur), r, _ptr(nrm), _ptr(dev['scale']), _ptr(A), A.shape[0],
                                       _ptr(out), n, None)
    _lib.check(rc, 'spr_project_field_f64')
    return eng.to_host(Ur), (eng.to_host(nrm) if norms else None), eng.to_host(out)


@pytest.mark.parametrize('n_points,F,m,r,row0,n_rows', SHAPES)
def test_against_long_double(eng, n_points, F, m, r, row0, n_rows):
    """The launch with norms and field: Ur against the long-double projection; norms and field against long-double sums
    over the basis AS STORED (what both are defined on)."""
    host, dev = _case(eng, n_points, F, m, r, row0, n_rows)
    Ur, nrm, field = _field_call(eng, dev, host['row0'], n_points, F)
    assert np.all(np.isfinite(Ur)) and np.all(np.isfinite(nrm)) and np.all(np.isfinite(field))
    err_u = np.abs(Ur.astype(LD) - host['Ur_ref']).astype(np.float64)
    print(f'Ur: max err / bound {np.max(err_u / host["bound_u"]):.3f}')
    assert np.all(err_u <= host['bound_u'])
    sq = np.sum(Ur.astype(LD) ** 2, axis=1)
    err_n = np.abs(nrm.astype(LD) - sq).astype(np.float64)
    print(f'norms: max err / bound {np.max(err_n / (2 * (r + 2) * EPS * sq.astype(np.float64))):.3f}')
    assert np.all(err_n <= 2 * (r + 2) * EPS * sq.astype(np.float64))
    sc, mean_h, a = host['scale'][host['feat']], host['mean'], host['a'][0]
    want = sc.astype(LD) * (Ur.astype(LD) @ a.astype(LD)) + mean_h.astype(LD)
    bound_f = 2 * (r + 2) * EPS * (sc * (np.abs(Ur) @ np.abs(a)) + np.abs(mean_h))
    err_f = np.abs(field[0].astype(LD) - want).astype(np.float64)
    print(f'field: max err / bound {np.max(err_f / bound_f):.3f}')
    assert np.all(err_f <= bound_f)


@pytest.mark.parametrize('n_points,F,m,r,row0,n_rows', SHAPES)
def test_four_epilogues_agree_bitwise(eng, n_points, F, m, r, row0, n_rows):
    """With and without the norm vector, with and without the field: the same Ur, the same norms, the same field; and the
    field equals the stand-alone reconstruct on the stored basis."""
    import torch
    host, dev = _case(eng, n_points, F, m, r, row0, n_rows)
    row0 = host['row0']
    Ur, nrm, field = _field_call(eng, dev, row0, n_points, F)
    Ur_b, _, field_b = _field_call(eng, dev, row0, n_points, F, norms=False)
    assert np.array_equal(Ur_b, Ur) and np.array_equal(field_b, field)
    X = dev['X']
    assert eng.project_field_max(X, r) > 0                           # the plain entry points take the same kernel here
    nrm_c = torch.full((host['n'],), float('nan'), dtype=torch.float64, device=X.device)
    Ur_c = eng.project(X, row0, n_points, F, dev['inv'], dev['W'], rowmean=dev['mean'], norms=nrm_c)
    assert np.array_equal(eng.to_host(Ur_c), Ur) and np.array_equal(eng.to_host(nrm_c), nrm)
    Ur_d = eng.project(X, row0, n_points, F, dev['inv'], dev['W'], rowmean=dev['mean'])
    assert np.array_equal(eng.to_host(Ur_d), Ur)
    plain = eng.reconstruct(Ur_d.contiguous(), row0, n_points, F, dev['mean'], dev['scale'], dev['a'])
    assert np.array_equal(eng.to_host(plain), field)


@pytest.mark.parametrize('m,r', [(256, 64), (256, 48), (128, 32), (192, 64)])
def test_feature_alone_equals_middle_feature(eng, m, r):
    """The rows of one feature give the same bits whether they are projected alone or as the middle feature of a
    three-feature matrix with equal scales: a row's arithmetic does not depend on the workgroup or the 16-row block it
    falls into (at n_points = 1371 the middle feature starts at row 11 of a block)."""
    n_points = 1371
    rng = np.random.default_rng(m + r)
    X3 = rng.standard_normal((3 * n_points, m)) * 2.0 + 1.0
    mean3 = X3.mean(axis=1)
    Wh = rng.standard_normal((m, r)) / np.sqrt(m)
    a_h = rng.standard_normal((1, r))
    common = dict(W=eng.to_device(Wh), a=eng.to_device(a_h))
    three = dict(common, X=eng.to_device(X3), mean=eng.to_device(mean3), inv=eng.to_device(np.full(3, 0.75)),
                 scale=eng.to_device(np.full(3, 1.5)))
    mid = slice(n_points, 2 * n_points)
    alone = dict(common, X=eng.to_device(np.ascontiguousarray(X3[mid])), mean=eng.to_device(np.ascontiguousarray(mean3[mid])),
                 inv=eng.to_device(np.full(1, 0.75)), scale=eng.to_device(np.full(1, 1.5)))
    Ur3, nrm3, field3 = _field_call(eng, three, 0, n_points, 3)
    Ur1, nrm1, field1 = _field_call(eng, alone, 0, n_points, 1)
    assert np.all(np.isfinite(Ur1)) and np.all(np.isfinite(nrm1)) and np.all(np.isfinite(field1))
    assert np.array_equal(Ur3[mid], Ur1)
    assert np.array_equal(nrm3[mid], nrm1)
    assert np.array_equal(field3[:, mid], field1)
