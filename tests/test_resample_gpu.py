"""csrc/resample.hip on the device, held to the brute-force oracle of tests/test_resample_host.py.  Every case runs twice and
the two results are compared bit for bit.

Bars (derived, not measured):
  * index, the -1 slots and valid equal the oracle's exactly (the random inputs have no near-tie, the lattice d2 are exact);
  * d2 is within 8 eps relative of the oracle's: one rounding per difference, square and sum;
  * 'idw' weights are within (k + 16) eps relative: the d2 error twice, the reciprocals, a k-term sum, a division;
  * 'nearest' application: the bytes of the oracle's row copy (the input holds NaN and -0.0), fill_value 0.0 and NaN;
  * 'idw' application: |out - oracle| <= (2 k + 16) eps sum_j w_j |x_j|, plus 2^-24 |out| for float32 storage (the one
    rounding on store); an entry whose sources hold a NaN is NaN on both sides.
The worst error / bar ratio of every case is printed (pytest -s shows it)."""
import numpy as np
import pytest

from openmeasure_amd.sparse_sensing import SPR, DeviceCSR, DeviceMatrix
from openmeasure_amd.utils import Resampler, resample_to_grid
from tests.test_raycast_host import notebook_camera
from tests.test_resample_host import (EPS, LD, RANDOM_CASES, centres, edge_cases, lattice_sources, lattice_targets,
                                      oracle_apply, oracle_neighbours, random_sources, snapshot_block, target_grid)

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope='module')
def eng():
    from openmeasure_amd.engine import HipEngine
    return HipEngine('cuda:0')


def host(eng, t):
    return np.array(eng.to_host(t.contiguous()))


def plan_twice(eng, src, dst, method, k, dmax):
    """-> (index, d2, weight, inspected) on the host, after a second search gave the same bits"""
    runs = []
    for _ in range(2):
        p = eng.resample_plan(np.array(src), dst, 1 if method == 'nearest' else k, method, dmax)
        runs.append(tuple(host(eng, p[key]) for key in ('index', 'd2', 'weight', 'inspected')))
    for x, y in zip(*runs):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
    assert [a.dtype for a in runs[0]] == [np.int64, np.float64, np.float64, np.int32]
    return runs[0]


def check_search(eng, src, dst, method, k, dmax, tag):
    k = 1 if method == 'nearest' else k
    q = centres(dst)
    index, d2, w, seen = plan_twice(eng, src, dst, method, k, dmax)
    oi, od, ow, _ = oracle_neighbours(src, q, k, method, dmax)
    assert index.shape == (len(q), k) and np.array_equal(index, oi), tag
    used = oi >= 0
    assert np.array_equal(index[:, 0] >= 0, used[:, 0]) and np.all(w[~used] == 0) and np.all(np.isinf(d2[~used])), tag
    with np.errstate(invalid='ignore', divide='ignore'):
        e_d = np.where(od[used] > 0, np.abs(d2[used] - od[used]) / od[used], np.abs(d2[used])) / (8 * EPS)
        e_w = np.where(ow[used] > 0, np.abs(w[used].astype(LD) - ow[used]) / ow[used], np.abs(w[used])).astype(np.float64) / ((k + 16) * EPS)
    worst = max(float(e_d.max(initial=0)), float(e_w.max(initial=0)))
    print(f'resample search {tag}: {len(src)} sources, {len(q)} targets, k = {k}, {np.count_nonzero(~used[:, 0])} invalid, '
          f'inspected mean {seen.mean():.1f} max {seen.max()}, worst error / bar: d2 {e_d.max(initial=0):.3f}, '
          f'weight {e_w.max(initial=0):.3f}')
    assert worst <= 1.0, tag
    assert np.all(seen >= np.minimum(k, used.sum(axis=1))) and np.all(seen <= len(src))
    WORST[f'search {tag}'] = worst
    return index, w


# ------------------------------------------------------------------------------------------------ search
@pytest.mark.parametrize('case', RANDOM_CASES)
@pytest.mark.parametrize('method,k', [('nearest', 1), ('idw', 3), ('idw', 8)])
def test_search_random(eng, case, method, k):
    src = random_sources(case)
    check_search(eng, src, target_grid(), method, k, None, f'{case} {method} {k} grid')
    if k == 8:                                                # the same targets as an explicit array: the same bits
        a = plan_twice(eng, src, target_grid(), method, k, None)
        b = plan_twice(eng, src, target_grid().cell_centers(), method, k, None)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize('method,k', [('nearest', 1), ('idw', 1), ('idw', 2), ('idw', 4), ('idw', 8)])
def test_search_lattice_ties(eng, method, k):
    check_search(eng, lattice_sources(), lattice_targets(), method, k, None, f'lattice {method} {k}')


@pytest.mark.parametrize('name', sorted(edge_cases()))
def test_search_edges(eng, name):
    src, dst, method, k, dmax = edge_cases()[name]
    check_search(eng, src, dst, method, k, dmax, name)


# ------------------------------------------------------------------------------------------------ application
@pytest.fixture(scope='module')
def operators(eng):
    """index / weight device tensors for n_src = 3000 and the 560 targets: name -> (method, k, index, weight, host copies)"""
    src, grid = random_sources('uniform'), target_grid()
    out = {}
    for name, (method, k, dmax) in {'nearest': ('nearest', 1, None), 'nearest dmax': ('nearest', 1, 0.12), 'idw 3': ('idw', 3, None),
                                    'idw 8 dmax': ('idw', 8, 0.12), 'idw 1': ('idw', 1, None), 'idw 2': ('idw', 2, None),
                                    'idw 4': ('idw', 4, None)}.items():
        p = eng.resample_plan(src, grid, k, method, dmax)
        out[name] = (method, k, p['index'], p['weight'], host(eng, p['index']), host(eng, p['weight']))
    return out


def apply_twice(eng, Xd, index, weight, method, fill, ldo, m):
    """-> the (n_features n_dst, ldo) buffer on the host (columns beyond m keep their fill), after a second run gave the same bits"""
    t = eng.torch
    runs = []
    for _ in range(2):
        buf = t.full((2 * index.shape[0], ldo), -777.0, dtype=Xd.dtype, device=Xd.device)
        got = eng.resample_apply(Xd, 3000, 2, index, weight, method, fill, out=buf[:, :m])
        assert got.data_ptr() == buf.data_ptr()
        runs.append(host(eng, buf))
    assert runs[0].tobytes() == runs[1].tobytes()
    return runs[0]


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('m', [1, 2, 3, 64, 130])
def test_apply(eng, operators, m, dtype):
    t = eng.torch
    X = snapshot_block(2 * 3000, m, seed=m, dtype=dtype)
    worst = 0.0
    for pad in (0, 5 if m % 2 == 0 else 4):                   # leading dimensions equal to m, and larger and odd
        ldx, ldo = m + pad, m + (pad + 2 if pad else 0)
        assert pad == 0 or (ldx % 2 == 1 and ldo % 2 == 1)
        wide = t.zeros((2 * 3000, ldx), dtype=t.float32 if dtype == np.float32 else t.float64, device=eng.device)
        wide[:, :m] = eng.to_device(X, dtype=wide.dtype)
        Xd = wide[:, :m]
        for name, (method, k, index, weight, hi, hw) in operators.items():
            for fill in (0.0, np.nan) if 'dmax' in name else (0.0,):
                got = apply_twice(eng, Xd, index, weight, method, fill, ldo, m)
                assert np.all(got[:, m:] == -777.0), (name, m, pad)          # the columns beside the block keep their bytes
                got = np.ascontiguousarray(got[:, :m])
                if method == 'nearest':
                    assert got.tobytes() == oracle_apply(X, 3000, 2, hi, hw, method, fill)[0].tobytes(), (name, m, pad, fill)
                    continue
                # the reference is NOT rounded to the storage type: the bar's 2^-24 |out| is that one rounding
                want, scale = oracle_apply(X.astype(np.float64), 3000, 2, hi, hw, method, fill)
                nan = np.isnan(want)
                assert np.array_equal(np.isnan(got), nan), (name, m, pad)
                bar = (2 * k + 16) * EPS * scale + (2.0 ** -24 * np.abs(want) if dtype == np.float32 else 0.0)
                err = np.abs(got.astype(np.float64) - want)
                ok = ~nan & (bar > 0)
                assert np.all(err[~nan & (bar == 0)] == 0)
                worst = max(worst, float((err[ok] / bar[ok]).max(initial=0)))
                assert np.all(err[ok] <= bar[ok]), (name, m, pad, float((err[ok] / bar[ok]).max()))
    print(f'resample apply m = {m} {np.dtype(dtype).name}: worst error / bar = {worst:.3f}')
    WORST[f'apply {m} {np.dtype(dtype).name}'] = worst


def test_apply_through_the_public_surface(eng, operators):
    """ndarray in / out, a device tensor, an out= that is a column block of a wider tensor, the operator as a matrix"""
    src, grid = random_sources('uniform'), target_grid()
    X = snapshot_block(2 * 3000, 6, seed=9)
    rs = Resampler(src, grid, engine=eng)
    assert rs.info_['n_invalid'] == 0 and rs.info_['inspected_max'] <= 3000 and bool(rs.valid.all())
    Y = rs.apply(X, 2)
    hi = host(eng, rs.index)
    assert isinstance(Y, np.ndarray) and Y.tobytes() == oracle_apply(X, 3000, 2, hi, None, 'nearest')[0].tobytes()
    t = eng.torch
    common = t.full((1120, 9), 3.25, dtype=t.float64, device=eng.device)
    rs.apply(eng.to_device(X), 2, out=common[:, 2:8])
    back = host(eng, common)
    assert back[:, 2:8].tobytes() == Y.tobytes() and np.all(back[:, :2] == 3.25) and np.all(back[:, 8:] == 3.25)
    idw = Resampler(src, grid, method='idw', k=4, engine=eng)
    C = idw.operator(to_host=False)
    assert isinstance(C, DeviceCSR) and C.shape == (560, 3000) and C.nnz == 4 * 560
    x = np.random.default_rng(1).standard_normal(3000)
    got = idw.apply(x, 1)
    assert got.shape == (560,) and np.allclose(got, C.tocsr() @ x, rtol=0, atol=64 * EPS * np.abs(x).max())


# ------------------------------------------------------------------------------------------------ the chain
def test_chain_resample_fit_project_train(eng):
    """xyz, X -> X_int on a VoxelGrid -> SPR -> camera.project -> train, the snapshot matrix never leaving HBM"""
    from tests.test_raycast_host import camera_grid
    grid = camera_grid()
    rng = np.random.default_rng(11)
    lo, hi = grid.corners()
    xyz = lo + (hi - lo) * rng.random((1500, 3))
    A = rng.standard_normal((4, 10))
    X = np.concatenate([np.cos(3 * xyz @ rng.standard_normal((3, 4))) @ A, 20 * np.sin(2 * xyz @ rng.standard_normal((3, 4))) @ A])
    g, X_int, xyz_int = resample_to_grid(xyz, DeviceMatrix(eng.to_device(X)), grid, engine=eng)
    assert g is grid and isinstance(X_int, DeviceMatrix) and X_int.shape == (2 * grid.n_cells, 10)
    idx = oracle_neighbours(xyz, grid.cell_centers(), 1)[0]
    want, _ = oracle_apply(X, 1500, 2, idx, None, 'nearest')
    assert host(eng, X_int.tensor).tobytes() == want.tobytes()
    spr = SPR(X_int, 2, xyz_int, engine=eng)
    spr.fit(select_modes='number', n_modes=4)
    C = notebook_camera().project(grid, feature=1, n_features=2, to_host=False, engine=eng)
    spr.train(C)
    Theta = np.asarray(spr.Theta)
    assert Theta.shape == (64, 4) and np.allclose(Theta, C.tocsr() @ np.asarray(spr.Ur), rtol=0, atol=1e-12 * np.abs(Theta).max())
    y = np.zeros((64, 3))
    y[:, 0] = C.dot(want[:, 3])
    y[:, 2] = 1
    Ar, _ = spr.predict(y)
    assert np.all(np.isfinite(np.asarray(spr.reconstruct(Ar))))


def test_zz_worst_ratio_overall():
    """the figure DESIGN.md records; runs last in this file"""
    if WORST:
        print('resample worst error / bar over all cases:', f'{max(WORST.values()):.3f}', 'in', max(WORST, key=WORST.get))
        assert max(WORST.values()) <= 1.0
