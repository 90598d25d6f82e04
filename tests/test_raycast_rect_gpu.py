"""The rectilinear kernels of csrc/raycast.hip on the device (spr_raycast_count_rect_f64 / spr_raycast_fill_rect_f64 behind
HipEngine.raycast), held to the brute-force longdouble oracle for stored edges of tests/test_raycast_rect_host.py.  Every case is
cast twice and the two results are compared bit for bit.

The contract and its bars are those of tests/test_raycast_gpu.py, unchanged (chord_bar is imported, not restated): a chord is
still a difference of two t = (plane - a) / d times |b - a|, and the plane is now an exact load where it was a rounded fma.
  * the cells of every segment, and of every pixel, equal the oracle's exactly and ascend in every row;
  * a chord is within chord_bar of the oracle's; the chords of a segment sum to its clipped length within bar x cells;
  * weights='hit' gives 1 everywhere, with col0 applied;
  * a pixel's mean chord is within the largest bar of its rays plus n_ray eps times the value.
Condition on the inputs (no tolerance), asserted here and in the host file: the smallest chord of a case is at least 1e-9 S.
The worst error / bar ratio of every case is printed (pytest -s shows it)."""
import numpy as np
import pytest

from openmeasure_amd.sparse_sensing import SPR, DeviceCSR
from openmeasure_amd.utils import RectilinearGrid, Resampler, VoxelGrid, resample_to_grid
from tests.test_raycast_gpu import cast_twice, hand_segments
from tests.test_raycast_host import EPS, chord_bar, coordinate_scale, field_of_rank, margin, notebook_camera, oracle_csr
from tests.test_raycast_rect_host import (CAMERA_CASES, DYADIC, HAND_NAMES, camera_case, camera_records, dyadic_segments,
                                          edge_oracle_segments, hand_grids, hand_records, stretched_camera_grid)

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope='module')
def eng():
    from openmeasure_amd.engine import HipEngine
    return HipEngine('cuda:0')


def check_case(eng, seg, grid, n_ray, recs, tag):
    """the whole contract for one set of segments and their oracle records; -> worst error / bar"""
    S = coordinate_scale(seg, grid)
    ip0, ix0, v0, _ = oracle_csr(seg, grid, 1, 'length', recs=recs)
    assert margin(recs, S) >= 1e-9, f'{tag}: a case near a grazing ray'
    worst = 0.0
    # per segment: n_ray = 1 makes every segment a row, weights='length' its chords
    ip, ix, v = cast_twice(eng, seg, grid, 1, 'length')
    assert np.array_equal(ip, ip0) and np.array_equal(ix, ix0), tag
    for s, rec in enumerate(recs):
        lo, hi = ip[s], ip[s + 1]
        if hi == lo:
            continue
        assert np.all(np.diff(ix[lo:hi]) > 0)
        bar = chord_bar(rec, S)
        err = np.abs(v[lo:hi].astype(np.longdouble) - rec['chords'])
        tot = abs(np.sum(v[lo:hi].astype(np.longdouble)) - rec['clipped'])
        worst = max(worst, float(err.max() / bar), float(tot / (bar * (hi - lo))))
        assert err.max() <= bar and tot <= bar * (hi - lo), (tag, s, float(err.max()), float(tot), bar)
    hp, hx, hv = cast_twice(eng, seg, grid, 1, 'hit', col0=7)
    assert np.array_equal(hp, ip0) and np.array_equal(hx, ix0 + 7) and np.all(hv == 1.0), tag
    if n_ray > 1:                                             # per pixel: the union of its rays, the mean chord
        bars = np.array([chord_bar(rec, S) if len(rec['cells']) else 0.0 for rec in recs]).reshape(-1, n_ray).max(axis=1)
        pp, px, pv, _ = oracle_csr(seg, grid, n_ray, 'length', recs=recs)
        ip, ix, v = cast_twice(eng, seg, grid, n_ray, 'length')
        assert np.array_equal(ip, pp) and np.array_equal(ix, px), tag
        for p in range(len(pp) - 1):
            lo, hi = pp[p], pp[p + 1]
            if hi == lo:
                continue
            assert np.all(np.diff(ix[lo:hi]) > 0)
            bar = bars[p] + n_ray * EPS * pv[lo:hi]
            err = np.abs(v[lo:hi] - pv[lo:hi])
            worst = max(worst, float((err / bar).max()))
            assert np.all(err <= bar), (tag, p, float(err.max()))
        hp, hx, hv = cast_twice(eng, seg, grid, n_ray, 'hit')
        assert np.array_equal(hp, pp) and np.array_equal(hx, px) and np.all(hv == 1.0), tag
    print(f'raycast rect {tag}: {len(seg)} segments, {len(ix0)} hits, margin {margin(recs, S):.2e} S, '
          f'worst error / bar = {worst:.3f}')
    WORST[tag] = worst
    return worst


# ------------------------------------------------------------------------------------------------ hand-made segments
@pytest.mark.parametrize('n_seg', [1, 63, 65, 257])
@pytest.mark.parametrize('name', HAND_NAMES)
def test_hand_made_segments(eng, name, n_seg):
    grid, seg, recs = hand_records(name)
    check_case(eng, seg[:n_seg], grid, 1, recs[:n_seg], f'{name} {n_seg}')
    if n_seg == 257:                                          # the expected empties are empty
        ip = cast_twice(eng, seg, grid, 1, 'hit')[0]
        assert np.all(np.diff(ip)[17:20] == 0) and np.all(np.diff(ip)[:17] > 0)


def test_the_edges_are_uploaded_once_per_engine(eng):
    grid = hand_grids()['stretched']
    assert grid._device_edges is None
    eng.raycast(hand_segments()[:5], grid, 1)
    cached = grid._device_edges
    assert cached[0] is eng and [tuple(e.shape) for e in cached[1]] == [(6,), (5,), (4,)]
    eng.raycast(hand_segments()[:5], grid, 1)
    assert grid._device_edges is cached
    for e, h in zip(cached[1], grid.edges):
        assert np.array_equal(np.array(eng.to_host(e)), h)


def test_no_ray_meets_the_grid(eng, monkeypatch):
    """an empty CSR, and no fill launch"""
    fills = []
    monkeypatch.setattr(eng, 'raycast_fill', lambda *a, **k: fills.append(a))
    for name in HAND_NAMES:
        ip, ix, v = cast_twice(eng, hand_segments()[17:20], hand_grids()[name], 3, 'hit')
        assert ip.tolist() == [0, 0] and ix.shape == (0,) and v.shape == (0,)
    assert not fills


# ------------------------------------------------------------------------------------------------ against the uniform kernels
def test_agreement_with_the_uniform_kernel(eng):
    """the same cells from both traversals on a grid whose planes origin + k * spacing are exact in NumPy's arithmetic and in
    the kernel's fma; chords within the bar of either.  Whether the chords agree bit for bit is printed, not asserted."""
    v = VoxelGrid(**DYADIC)
    g = RectilinearGrid.from_voxel_grid(v)
    seg = dyadic_segments()
    recs = edge_oracle_segments(seg, g)
    S = coordinate_scale(seg, g)
    assert margin(recs, S) >= 1e-9
    ipu, ixu, vu = cast_twice(eng, seg, v, 1, 'length')
    ipr, ixr, vr = cast_twice(eng, seg, g, 1, 'length')
    assert np.array_equal(ipu, ipr) and np.array_equal(ixu, ixr) and len(ixr) > 500
    worst = 0.0
    for s, rec in enumerate(recs):
        lo, hi = ipr[s], ipr[s + 1]
        if hi > lo:
            bar = chord_bar(rec, S)
            worst = max(worst, float(np.abs(vu[lo:hi] - vr[lo:hi]).max() / bar))
            assert np.all(np.abs(vu[lo:hi] - vr[lo:hi]) <= bar), s
    print(f'raycast rect against uniform: {len(ixr)} hits, chords bit for bit: {vu.tobytes() == vr.tobytes()} '
          f'({int(np.count_nonzero(vu != vr))} differ), worst difference / bar = {worst:.3f}')
    check_case(eng, seg, g, 1, recs, 'dyadic')


# ------------------------------------------------------------------------------------------------ cameras
@pytest.mark.parametrize('case', CAMERA_CASES)
def test_cameras(eng, case):
    """the cameras of tests/test_raycast_gpu.py through stretched_camera_grid(), graded by 1.3; every case passes the 1e-9
    margin with the seed of the uniform test, so neither the ratio nor a seed had to be changed"""
    cam, type_rec = camera_case(case)
    grid, seg, n_ray, recs = camera_records(case)
    assert n_ray == (1 if type_rec == 'parallel' else 3)
    check_case(eng, seg, grid, n_ray, recs, f'camera {case}')
    # the public route gives the same matrix
    C = cam.project(grid, type_rec, N_rand=3, seed=5, weights='length', feature=1, n_features=2, to_host=False, engine=eng)
    ip, ix, v = cast_twice(eng, seg, grid, n_ray, 'length', col0=grid.n_cells)
    H = C.tocsr()
    assert isinstance(C, DeviceCSR) and C.shape == (64, 480)
    assert np.array_equal(H.indptr, ip) and np.array_equal(H.indices, ix) and np.array_equal(H.data, v)


# ------------------------------------------------------------------------------------------------ resampling onto the grid
@pytest.mark.parametrize('method,k', [('nearest', 1), ('idw', 4)])
def test_resampler_onto_a_rectilinear_grid(eng, method, k):
    grid = hand_grids()['stretched']
    rng = np.random.default_rng(11)
    src = rng.uniform(grid.corners()[0] - 0.3, grid.corners()[1] + 0.3, size=(500, 3))
    X = rng.standard_normal((3 * 500, 6))
    a = Resampler(src, grid, method=method, k=k, engine=eng)
    b = Resampler(src, grid.cell_centers(), method=method, k=k, engine=eng)
    assert a.n_dst == 60 and tuple(a.index.shape) == (60, k)
    for p, q in zip((a.index, a.weight, a.d2), (b.index, b.weight, b.d2)):
        assert np.array(eng.to_host(p)).tobytes() == np.array(eng.to_host(q)).tobytes()
    out_grid, X_int, xyz_int = resample_to_grid(src, X, grid, method=method, k=k, engine=eng)
    assert out_grid is grid and np.array_equal(xyz_int, grid.cell_centers())
    assert isinstance(X_int, np.ndarray) and X_int.shape == (3 * 60, 6) and X_int.tobytes() == a.apply(X, 3).tobytes()
    X_dev = resample_to_grid(src, eng.to_device(X), grid, method=method, k=k, engine=eng)[1]     # stays in HBM
    assert isinstance(X_dev, eng.torch.Tensor) and X_dev.is_cuda and np.array(eng.to_host(X_dev)).tobytes() == X_int.tobytes()


# ------------------------------------------------------------------------------------------------ camera -> C -> train -> predict
def test_end_to_end_camera_train_predict_reconstruct(eng):
    """The end-to-end test of tests/test_raycast_gpu.py on stretched_camera_grid() (field_of_rank reads n_cells alone): x_j lies
    in the span of the 4 modes, cond(Theta) <= 1e3 is asserted from the host twin C Ur, and the bar is that test's 1e-8."""
    grid = stretched_camera_grid()
    X = field_of_rank(grid)
    spr = SPR(X, 2, grid.cell_centers(), engine=eng)
    spr.fit(select_modes='number', n_modes=4)
    C = notebook_camera().project(grid, feature=1, n_features=2, to_host=False, engine=eng)
    assert isinstance(C, DeviceCSR) and C.shape == (64, 480) and C.nnz == 240
    spr.train(C)
    Theta = np.array(spr.Theta)
    H = C.tocsr()
    twin = H @ np.asarray(spr.Ur)
    sv = np.linalg.svd(twin, compute_uv=False)
    cond = sv[0] / sv[-1]
    assert Theta.shape == (64, 4) and cond <= 1e3 and np.allclose(Theta, twin, rtol=0, atol=1e-12 * sv[0])
    worst = 0.0
    for j in (0, 7):
        y = np.zeros((64, 3))
        y[:, 0] = C.dot(X[:, j])
        assert np.allclose(y[:, 0], H @ X[:, j], rtol=1e-13, atol=1e-13 * np.abs(X[:, j]).max())
        y[:, 2] = 1
        Ar, _ = spr.predict(y)
        xr = np.asarray(spr.reconstruct(Ar)).reshape(-1)
        rel = np.linalg.norm(xr - X[:, j]) / np.linalg.norm(X[:, j])
        worst = max(worst, rel)
        assert rel <= 1e-8, (j, rel)
    print(f'raycast rect end to end: cond(Theta) = {cond:.1f}, worst relative error of the field = {worst:.2e}')


def test_zz_worst_ratio_overall():
    """the figure DESIGN.md records; runs last in this file"""
    if WORST:
        print('raycast rect worst error / bar over all cases:', f'{max(WORST.values()):.3f}', 'in', max(WORST, key=WORST.get))
        assert max(WORST.values()) <= 1.0
