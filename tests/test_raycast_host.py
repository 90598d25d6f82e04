"""The tomography front end on the CPU: openmeasure_amd.utils (VoxelGrid, camera), DeviceCSR and train(DeviceCSR) over a
NumPy double of the engine's ray caster, the brute-force oracle both this file and tests/test_raycast_gpu.py hold the device
kernels to, and the parity of camera.segments with the UNMODIFIED reference camera through a recorded fixture.

Oracle: for every segment and every cell its bounding box reaches the slab test in np.longdouble on the same float64 end points: the cell's box
clips [0, 1] to [t_enter, t_exit]; a hit is t_exit > t_enter, its chord (t_exit - t_enter) |b - a|.  No traversal, no
shared code with csrc/raycast.hip.

Fixture: tests/golden/camera_segments.json is written by tools/make_camera_record.py, which runs the reference's
camera.project over a stand-in mesh that records the end points it is asked about (and the uniform numbers drawn).
camera(...) and camera.segments(draws=...) are held to it at 4 eps of the coordinate scale: both sides evaluate the same
formulas in float64, in another order of operations (one matrix product for all rays instead of one per ray)."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from openmeasure_amd.sparse_sensing import SPR, DeviceCSR
from openmeasure_amd.utils import VoxelGrid, camera, resample_to_grid
from tests.numpy_engine import NumpyEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'camera_segments.json')
LD = np.longdouble
EPS = 2.0 ** -52


# ------------------------------------------------------------------------------------------------ the oracle
def _slab(a, d, lo, hi):
    """t-interval in which a + t d lies strictly inside (lo, hi); lo / hi arrays, a / d longdouble scalars"""
    if d == 0:
        inside = (lo < a) & (a < hi)
        return np.where(inside, -np.inf, np.inf).astype(LD), np.where(inside, np.inf, -np.inf).astype(LD)
    t1, t2 = (lo - a) / d, (hi - a) / d
    return np.minimum(t1, t2), np.maximum(t1, t2)


def _boxes(grid, lo_idx=(0, 0, 0), hi_idx=None):
    """(ids, lo, hi) of the cells with indices lo_idx <= (i, j, k) <= hi_idx: boxes (n, 3) in longdouble, ascending ids"""
    o, h = np.asarray(grid.origin, dtype=LD), np.asarray(grid.spacing, dtype=LD)
    nx, ny, nz = grid.dims
    hi_idx = (nx - 1, ny - 1, nz - 1) if hi_idx is None else hi_idx
    k, j, i = np.meshgrid(*(np.arange(lo_idx[d], hi_idx[d] + 1) for d in (2, 1, 0)), indexing='ij')
    idx = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1)
    ids = idx[:, 0] + nx * (idx[:, 1] + ny * idx[:, 2])
    return ids.astype(np.int64), o + idx.astype(LD) * h, o + (idx.astype(LD) + 1) * h


def oracle_segments(seg, grid):
    """seg (n, 6) float64 -> list of dicts per segment: cells (ascending ids), chords (longdouble), length |b - a|,
    clipped (length inside the whole grid), cross (axes in which the clipped part meets a cell plane)"""
    o, h = np.asarray(grid.origin, dtype=LD), np.asarray(grid.spacing, dtype=LD)
    glo, ghi = o[None, :], (o + np.asarray(grid.dims, dtype=LD) * h)[None, :]
    out = []
    for s in np.asarray(seg, dtype=np.float64):
        a, d = s[:3].astype(LD), s[3:].astype(LD) - s[:3].astype(LD)
        L = np.sqrt(np.sum(d * d))

        def clip(lo, hi):
            te, tx = np.zeros(len(lo), dtype=LD), np.ones(len(lo), dtype=LD)
            for ax in range(3):
                e, x = _slab(a[ax], d[ax], lo[:, ax], hi[:, ax])
                te, tx = np.maximum(te, e), np.minimum(tx, x)
            return te, tx

        if L == 0:
            out.append(dict(cells=np.zeros(0, dtype=np.int64), chords=np.zeros(0, dtype=LD), length=L, clipped=LD(0), cross=[]))
            continue
        # every cell the segment's bounding box reaches, one more on every side (a cell outside that box cannot be hit)
        f = [np.floor((s[[ax, ax + 3]] - grid.origin[ax]) / grid.spacing[ax]) for ax in range(3)]
        first = [int(np.clip(f[ax].min() - 1, 0, grid.dims[ax] - 1)) for ax in range(3)]
        last = [int(np.clip(f[ax].max() + 1, 0, grid.dims[ax] - 1)) for ax in range(3)]
        ids, lo, hi = _boxes(grid, first, last)
        te, tx = clip(lo, hi)
        hit = np.flatnonzero(tx > te)
        g0, g1 = clip(glo, ghi)
        clipped = (g1[0] - g0[0]) * L if g1[0] > g0[0] else LD(0)
        cross = []
        if clipped > 0:
            for ax in range(3):
                c0, c1 = sorted((a[ax] + g0[0] * d[ax], a[ax] + g1[0] * d[ax]))
                planes = o[ax] + np.arange(grid.dims[ax] + 1, dtype=LD) * h[ax]
                slack = LD(1e-12) * max(abs(c0), abs(c1), 1e-300)
                if d[ax] != 0 and np.any((planes >= c0 - slack) & (planes <= c1 + slack)):
                    cross.append(ax)
        out.append(dict(cells=ids[hit], chords=((tx - te) * L)[hit], length=L, clipped=clipped, cross=cross,
                        d=d))
    return out


def coordinate_scale(seg, grid):
    """S: the largest absolute coordinate among the end points and the grid corners"""
    return float(max(np.max(np.abs(seg)) if len(seg) else 0.0, np.max(np.abs(grid.corners()))))


def chord_bar(rec, S):
    """64 eps S max(|b - a| / |d_ax|) over the axes the clipped segment crosses a cell plane in.  Every chord is a difference
    of two parameters t = (plane - a_ax) / d_ax times |b - a|: plane and a_ax are coordinates of size <= S known to eps S, so t
    carries eps S / |d_ax| per operation and the chord eps S |b - a| / |d_ax|; 64 covers the handful of operations (plane, two
    differences, division, the clip's max / min, the product with the rounded norm).  A segment that meets no plane lies in
    one cell with t = 0 .. 1 exact: the factor is 1."""
    f = max([float(rec['length'] / abs(rec['d'][ax])) for ax in rec['cross']], default=1.0)
    return 64 * EPS * S * f


def oracle_csr(seg, grid, n_ray, weights='hit', col0=0, recs=None):
    """The CSR rows of the pixels: (indptr, indices, vals) as NumPy arrays -- union of the pixel's rays, vals 1 or the mean
    chord -- and the per-segment records"""
    recs = oracle_segments(seg, grid) if recs is None else recs
    n_pix = len(recs) // n_ray
    indptr, indices, vals = [0], [], []
    for p in range(n_pix):
        acc = {}
        for rec in recs[p * n_ray:(p + 1) * n_ray]:
            for c, ch in zip(rec['cells'], rec['chords']):
                acc[int(c)] = acc.get(int(c), LD(0)) + ch
        for c in sorted(acc):
            indices.append(c + col0)
            vals.append(1.0 if weights == 'hit' else float(acc[c] / n_ray))
        indptr.append(len(indices))
    return np.array(indptr, dtype=np.int64), np.array(indices, dtype=np.int64), np.array(vals, dtype=np.float64), recs


class OracleRaycastEngine(NumpyEngine):
    """NumpyEngine whose raycast is the oracle, with the contract of HipEngine.raycast; counts its calls"""

    def __init__(self):
        super().__init__()
        self.raycast_calls = 0
        self.measure_calls = 0

    def raycast(self, segments, grid, n_ray, weights='hit', col0=0):
        assert isinstance(segments, np.ndarray) and segments.dtype == np.float64 and segments.ndim == 2
        assert segments.shape[1] == 6 and segments.shape[0] % n_ray == 0 and np.all(np.isfinite(segments))
        assert weights in ('hit', 'length')
        self.raycast_calls += 1
        indptr, indices, vals, _ = oracle_csr(segments, grid, n_ray, weights, col0)
        return torch.from_numpy(indptr), torch.from_numpy(indices), torch.from_numpy(vals)

    def measure_csr(self, *args, **kw):
        self.measure_calls += 1
        return super().measure_csr(*args, **kw)


# ------------------------------------------------------------------------------------------------ shared cases
def notebook_camera(tilt=(0.0, 0.0, 0.0), px=(8, 8), px_size=0.05, shift=(0.0, 0.0, 0.0)):
    """the notebook's orientation (cell 10): the camera sits on +x and looks along -x; image x runs along global y, image y
    along global z"""
    theta = np.array([-np.pi / 2, 0.0, -np.pi / 2]) + np.asarray(tilt, dtype=np.float64)
    return camera(np.array([1.0 + shift[0], shift[1], 0.3 + shift[2], 1.0]), theta, 1, 1, 1, np.array(px), px_size)


def pinhole_camera():
    """every pinhole ray passes through the lens centre, one unit in front of the camera: the notebook's position would put
    that point on a corner of camera_grid()'s cells, so this camera stands a little off"""
    return notebook_camera(shift=(0.013, 0.007, 0.011))


def camera_grid():
    """8 x 6 x 5 cells of 0.05 whose centres in y and z are pixel centres of notebook_camera()"""
    return VoxelGrid((-0.2, -0.15, 0.15), (0.05, 0.05, 0.05), (8, 6, 5))


def focused_camera():
    """m = 0.25: the thin-lens model applies.  Object plane at 0.9 in front of the lens, the grid of camera_grid() around it."""
    return camera(np.array([1.0, 0.0, 0.3, 1.0]), np.array([-np.pi / 2, 0.0, -np.pi / 2]), 0.18, 4.0, 0.225,
                  np.array([8, 8]), 0.0125)


def segments_of(cam, type_rec, N_rand=3, seed=5):
    a, b = cam.segments(type_rec, N_rand, seed=seed)
    return np.concatenate([a, b], axis=2).reshape(-1, 6), a.shape[1]


def margin(recs, S):
    """the smallest chord of any (segment, cell) hit over S"""
    ch = [float(rec['chords'].min()) for rec in recs if len(rec['chords'])]
    return min(ch) / S if ch else np.inf


# ------------------------------------------------------------------------------------------------ the oracle itself
def test_oracle_on_cases_known_by_hand():
    grid = VoxelGrid((0.0, 0.0, 0.0), (1.0, 2.0, 3.0), (3, 2, 2))
    seg = np.array([[-1.0, 1.0, 1.5, 4.0, 1.0, 1.5],          # along +x through the centres of cells 0, 1, 2
                    [0.5, 1.0, 1.5, 2.5, 1.0, 1.5],           # inside -> inside: half, whole, half a cell
                    [0.5, 5.0, 1.5, 2.5, 5.0, 1.5],           # outside the y slab
                    [0.5, 0.5, 0.5, 0.5, 0.5, 0.5]])          # a == b
    r = oracle_segments(seg, grid)
    assert r[0]['cells'].tolist() == [0, 1, 2] and np.allclose(r[0]['chords'].astype(float), 1.0)
    assert r[1]['cells'].tolist() == [0, 1, 2] and np.allclose(r[1]['chords'].astype(float), [0.5, 1.0, 0.5])
    assert r[0]['cross'] == [0] and float(r[0]['clipped']) == 3.0
    assert len(r[2]['cells']) == 0 and len(r[3]['cells']) == 0
    diag = oracle_segments(np.array([[0.25, 0.5, 0.75, 2.75, 3.5, 5.25]]), grid)[0]
    assert abs(float(diag['chords'].sum() - diag['clipped'])) < 1e-15 and diag['cross'] == [0, 1, 2]
    ip, ix, v, _ = oracle_csr(seg[[0, 1]], grid, 2, 'length', col0=12)
    assert ip.tolist() == [0, 3] and ix.tolist() == [12, 13, 14] and np.allclose(v, [0.75, 1.0, 0.75])


def test_the_camera_cases_stay_clear_of_grazing_rays():
    """the condition the GPU test puts on its inputs, checked here as well: margins of the cases both files use"""
    grid = camera_grid()
    for cam, type_rec in ((notebook_camera(), 'parallel'), (notebook_camera((0.09, 0.05, 0.12)), 'parallel'),
                          (pinhole_camera(), 'pinhole'), (focused_camera(), 'thin_lens')):
        seg, _ = segments_of(cam, type_rec)
        recs = oracle_segments(seg, grid)
        assert sum(len(r['cells']) for r in recs) > 0
        assert margin(recs, coordinate_scale(seg, grid)) >= 1e-9, type_rec


# ------------------------------------------------------------------------------------------------ parity with the reference
def _fixture_camera(s):
    p = s['parameters']
    return camera(np.array(p['p_cam']), np.array(p['theta']), p['f_length'], p['n_aper'], p['d_sensor'],
                  np.array(s['sensor_size_px']), p['px_size'])


def test_camera_matches_the_recorded_reference():
    rec = json.load(open(FIXTURE))
    assert len(rec['sets']) == 2 and sum(s['attributes']['m'] > 0 for s in rec['sets']) >= 1
    for s in rec['sets']:
        cam, at = _fixture_camera(s), s['attributes']
        assert cam.n_pixels == at['n_pixels'] == 12
        assert cam.d == at['d'] and cam.m == at['m'] and cam.d_object == at['d_object']
        assert np.array_equal(cam.sensor_size_m, at['sensor_size_m'])
        scale = max(1.0, float(np.max(np.abs(s['E']))))
        assert np.max(np.abs(cam._extr_matrix() - np.array(s['E']))) <= 4 * EPS * scale
        assert np.array_equal(cam._sensor_coordinates(), np.array(s['sensor_coordinates']))
        for type_rec, m in s['models'].items():
            if m is None:                                     # the reference refuses the thin lens at m = 0, and so do we
                assert type_rec == 'thin_lens' and cam.m == 0
                with pytest.raises(ValueError, match='focus at infinity'):
                    cam.segments('thin_lens', s['N_rand'])
                continue
            draws = {k: np.array(m[k]) for k in ('jitter', 'lens') if k in m}
            a, b = cam.segments(type_rec, s['N_rand'], draws=draws or None)
            ra, rb = np.array(m['a']), np.array(m['b'])
            assert a.shape == ra.shape == (12, 1 if type_rec == 'parallel' else 2, 3)
            S = max(np.max(np.abs(ra)), np.max(np.abs(rb)))
            assert np.max(np.abs(a - ra)) <= 4 * EPS * S and np.max(np.abs(b - rb)) <= 4 * EPS * S, type_rec


def _close_tree(x, y, tol):
    if isinstance(x, dict):
        return x.keys() == y.keys() and all(_close_tree(x[k], y[k], tol) for k in x)
    if isinstance(x, list) and (not x or isinstance(x[0], (dict, str))):
        return len(x) == len(y) and all(_close_tree(u, v, tol) for u, v in zip(x, y))
    if isinstance(x, list):
        ax, ay = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        return ax.shape == ay.shape and bool(np.all(np.abs(ax - ay) <= tol * np.maximum(1.0, np.abs(ay))))
    if isinstance(x, float) and isinstance(y, float):
        return abs(x - y) <= tol * max(1.0, abs(y))
    return x == y


def test_the_fixture_is_what_the_recipe_writes(tmp_path):
    """where the reference is present (the CPU box): the recipe, run again, gives the committed fixture"""
    ref = os.environ.get('OPENMEASURE_REFERENCE', '/root/reference/src')
    if not os.path.exists(os.path.join(ref, 'openmeasure', 'utils.py')):
        pytest.skip('the reference is not on this machine')
    out = tmp_path / 'camera_segments.json'
    subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'make_camera_record.py'), '--reference', ref, '--out', str(out)],
                   check=True, capture_output=True)
    assert _close_tree(json.load(open(out)), json.load(open(FIXTURE)), 4 * EPS)


def test_seeded_segments_repeat_and_thin_lens_uses_one_lens_point_per_pixel():
    cam = focused_camera()
    a1, b1 = cam.segments('thin_lens', 3, seed=11)
    a2, b2 = cam.segments('thin_lens', 3, seed=11)
    assert np.array_equal(a1, a2) and np.array_equal(b1, b2) and a1.shape == (64, 3, 3)
    assert np.array_equal(a1[:, 0], a1[:, 1]) and np.array_equal(a1[:, 0], a1[:, 2])    # the reference's quirk (:439)
    assert not np.array_equal(cam.segments('thin_lens', 3, seed=12)[1], b1)
    a, b = cam.segments('parallel', N_rand=99)
    assert a.shape == b.shape == (64, 1, 3)


# ------------------------------------------------------------------------------------------------ VoxelGrid
def test_voxel_grid():
    grid = VoxelGrid((-1.1, 0.3, -0.4), (0.5, 0.25, 1.0), (5, 4, 3))
    assert grid.n_cells == 60
    xyz = grid.cell_centers()
    assert xyz.shape == (60, 3)
    for cid, (i, j, k) in ((0, (0, 0, 0)), (1, (1, 0, 0)), (5, (0, 1, 0)), (20, (0, 0, 1)), (59, (4, 3, 2))):
        assert np.allclose(xyz[cid], [-1.1 + (i + .5) * .5, 0.3 + (j + .5) * .25, -0.4 + (k + .5) * 1.0], rtol=0, atol=1e-15)
    # the notebook's cell 9: float32 ranges, points of a structured grid
    dx = 0.2 / 32
    xr, yr, zr = (np.arange(lo, hi, dx, dtype=np.float32) for lo, hi in ((-0.1, 0.1), (-0.1, 0.1), (0.1, 0.5)))
    g = VoxelGrid.from_axes(xr, yr, zr)
    assert g.dims == (len(xr) - 1, len(yr) - 1, len(zr) - 1) and np.allclose(g.spacing, dx, rtol=1e-5)
    x, y, z = np.meshgrid(xr, yr, zr, indexing='ij')
    g3 = VoxelGrid.from_axes(x, y, z)
    assert g3.dims == g.dims and np.array_equal(g3.origin, g.origin) and np.array_equal(g3.spacing, g.spacing)
    with pytest.raises(ValueError, match='uniform'):
        VoxelGrid.from_axes(np.array([0.0, 1.0, 2.0001]), xr, xr)
    with pytest.raises(ValueError, match='indexing'):
        VoxelGrid.from_axes(*np.meshgrid(xr, yr, zr, indexing='xy'))
    for bad in (dict(origin=(0, 0, 0), spacing=(1, 0, 1), dims=(2, 2, 2)), dict(origin=(0, 0, 0), spacing=(1, 1, 1), dims=(2, 0, 2)),
                dict(origin=(0, np.nan, 0), spacing=(1, 1, 1), dims=(2, 2, 2)), dict(origin=(0, 0), spacing=(1, 1, 1), dims=(2, 2, 2))):
        with pytest.raises(ValueError):
            VoxelGrid(**bad)
    with pytest.raises(NotImplementedError):
        VoxelGrid((0, 0, 0), (1, 1, 1), (2048, 1024, 1024))


# ------------------------------------------------------------------------------------------------ project / DeviceCSR
def test_project_shapes_feature_block_and_engine_calls():
    import scipy.sparse as sp
    eng, grid, cam = OracleRaycastEngine(), camera_grid(), notebook_camera()
    C = cam.project(grid, engine=eng)
    assert sp.issparse(C) and C.format == 'csr' and C.shape == (64, 240) and eng.raycast_calls == 1
    # 6 x 5 pixels look through the grid, each through the 8 cells of a row along x; the others see nothing
    assert C.nnz == 30 * 8 and set(np.diff(C.indptr).tolist()) == {0, 8} and np.all(C.data == 1.0)
    xyz = grid.cell_centers()
    E_inv = np.linalg.inv(cam._extr_matrix())
    centres = (cam._sensor_coordinates() @ E_inv.T)[:, :3]
    for p in np.flatnonzero(np.diff(C.indptr)):
        cols = C.indices[C.indptr[p]:C.indptr[p + 1]]
        assert np.all(np.diff(cols) > 0)
        assert np.allclose(xyz[cols][:, 1:], centres[p, 1:], rtol=0, atol=1e-12)   # the cells behind the pixel centre
    D = cam.project(grid, feature=1, n_features=2, to_host=False, engine=eng)
    assert isinstance(D, DeviceCSR) and D.shape == (64, 480) and D.nnz == C.nnz and D.ndim == 2 and eng.raycast_calls == 2
    H = D.tocsr()
    assert np.array_equal(H.indptr, C.indptr) and np.array_equal(H.indices, C.indices + 240) and np.array_equal(H.data, C.data)
    W = cam.project(grid, weights='length', engine=eng)
    assert np.array_equal(W.indices, C.indices) and np.allclose(W.data, 0.05, rtol=1e-12)
    P = cam.project(grid, 'pinhole', N_rand=3, seed=2, engine=eng)
    P2 = cam.project(grid, 'pinhole', N_rand=3, seed=2, engine=eng)
    assert P.shape == (64, 240) and (P != P2).nnz == 0 and P.nnz > 0


def test_project_refusals():
    eng, grid, cam = OracleRaycastEngine(), camera_grid(), notebook_camera()
    with pytest.raises(ValueError, match='type_rec'):
        cam.project(grid, 'fisheye', engine=eng)
    with pytest.raises(ValueError, match='focus at infinity'):
        cam.project(grid, 'thin_lens', engine=eng)
    with pytest.raises(ValueError, match='weights'):
        cam.project(grid, weights='area', engine=eng)
    for feature, n_features in ((2, 2), (-1, 2), (0, 0)):
        with pytest.raises(ValueError, match='feature'):
            cam.project(grid, feature=feature, n_features=n_features, engine=eng)
    with pytest.raises(TypeError):
        cam.project(object(), engine=eng)
    with pytest.raises(ValueError, match='N_rand'):
        cam.project(grid, 'pinhole', N_rand=0, engine=eng)
    far = camera(np.array([np.inf, 0.0, 0.3, 1.0]), np.array([0.0, 0.0, 0.0]), 1, 1, 1, np.array([2, 2]), 0.1)
    with np.errstate(all='ignore'), pytest.raises(ValueError, match='finite'):
        far.project(grid, engine=eng)
    assert eng.raycast_calls == 0                             # every refusal came before the engine was asked
    with pytest.raises(NotImplementedError):
        cam.generate_camera()
    with pytest.raises(NotImplementedError):
        resample_to_grid(None, None, None)


def test_device_csr_dot_vstack_pickle():
    import scipy.sparse as sp
    eng, grid = OracleRaycastEngine(), camera_grid()
    A = notebook_camera().project(grid, 'pinhole', N_rand=2, seed=1, weights='length', to_host=False, engine=eng)
    B = notebook_camera((0.09, 0.05, 0.12)).project(grid, weights='length', to_host=False, engine=eng)
    x = np.random.default_rng(0).standard_normal(240)
    assert eng.measure_calls == 0
    y = A.dot(x)
    assert eng.measure_calls == 1 and y.shape == (64,) and np.allclose(y, A.tocsr() @ x, rtol=1e-13, atol=1e-15)
    with pytest.raises(ValueError):
        A.dot(np.zeros(239))
    V = DeviceCSR.vstack([A, B])
    assert V.shape == (128, 240) and V.nnz == A.nnz + B.nnz
    assert (V.tocsr() != sp.vstack([A.tocsr(), B.tocsr()]).tocsr()).nnz == 0
    assert np.allclose(V.dot(x), np.concatenate([A.dot(x), B.dot(x)]))
    wide = notebook_camera().project(grid, n_features=2, to_host=False, engine=eng)
    with pytest.raises(ValueError, match='column'):
        DeviceCSR.vstack([A, wide])
    with pytest.raises(ValueError):
        DeviceCSR.vstack([])
    R = pickle.loads(pickle.dumps(V))
    assert isinstance(R, DeviceCSR) and isinstance(R.indptr, np.ndarray) and R.shape == V.shape and R.nnz == V.nnz
    assert (R.tocsr() != V.tocsr()).nnz == 0
    R._engine(eng)                                            # an unpickled matrix is uploaded by whoever uses it first
    assert np.array_equal(R.dot(x), V.dot(x)) and isinstance(R.indptr, torch.Tensor)


def field_of_rank(grid, n_features=2, m=10, rank=4, seed=3):
    """m snapshots on the grid's cells, n_features features, of exact rank `rank` after centring"""
    rng = np.random.default_rng(seed)
    n = n_features * grid.n_cells
    A = rng.standard_normal((rank, m))
    A -= A.mean(axis=1, keepdims=True)
    X = rng.standard_normal((n, rank)) @ A + (3.0 + rng.standard_normal((n, 1)))
    X[grid.n_cells:] *= 20.0                                  # the second feature on another scale
    return X


def test_train_takes_a_device_csr():
    eng, grid = OracleRaycastEngine(), camera_grid()
    X = field_of_rank(grid)
    spr = SPR(X, 2, grid.cell_centers(), engine=eng)
    spr.fit(select_modes='number', n_modes=4)
    C = notebook_camera().project(grid, feature=1, n_features=2, to_host=False, engine=eng)
    assert eng.raycast_calls == 1
    spr.train(C)
    Theta = np.array(spr.Theta)
    assert spr.C is C and Theta.shape == (64, 4) and eng.measure_calls == 1
    spr.train(C.tocsr())
    assert np.array_equal(Theta, spr.Theta) and eng.raycast_calls == 1
    assert np.allclose(Theta, C.tocsr() @ spr.Ur, rtol=1e-12, atol=1e-14)
    spr.train(C)
    j = 4
    y = np.zeros((64, 3))
    y[:, 0] = C.dot(X[:, j])
    y[:, 2] = 1
    Ar, _ = spr.predict(y)
    xr = np.asarray(spr.reconstruct(Ar)).reshape(-1)
    assert np.linalg.norm(xr - X[:, j]) <= 1e-8 * np.linalg.norm(X[:, j])
    # sampled reconstruction and un-scaling take the same object
    assert np.array_equal(spr.reconstruct(Ar, sampling=C), spr.reconstruct(Ar, sampling=C.tocsr()))
    u = spr.unscale_data(np.zeros(64), sampling=C)
    assert np.allclose(np.asarray(u).reshape(-1), C.tocsr() @ spr.X_cnt.reshape(-1), rtol=1e-12)
    with pytest.raises(ValueError, match='columns'):
        spr.train(notebook_camera().project(grid, to_host=False, engine=eng))   # 240 columns against 480 rows


# ------------------------------------------------------------------------------------------------ sharded objects
def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from openmeasure_amd.sparse_sensing import SPR, RowShard
        from tests.test_raycast_host import OracleRaycastEngine, camera_grid, field_of_rank, notebook_camera
        grid = camera_grid()
        X = field_of_rank(grid)
        n = X.shape[0]
        cuts = [0, 300, n]                                    # cut inside the second feature (features of 240 rows)
        row0, n_loc = cuts[rank], cuts[rank + 1] - cuts[rank]
        eng = OracleRaycastEngine()
        spr = SPR(np.ascontiguousarray(X[row0:row0 + n_loc]), 2, None, shard=RowShard(row0, n), engine=eng)
        spr.fit(select_modes='number', n_modes=4)
        calls = []
        ag, ar = spr._all_gather, spr._all_reduce
        spr._all_gather = lambda t: (calls.append('gather'), ag(t))[1]
        spr._all_reduce = lambda t: (calls.append('reduce'), ar(t))[1]
        C = notebook_camera().project(grid, feature=1, n_features=2, to_host=False, engine=eng)   # global column ids
        built_with = len(calls)
        spr.train(C)
        np.savez(os.path.join(out_dir, f'rank{rank}.npz'), Theta=spr.Theta, built_with=built_with, indices=C.tocsr().indices)
    finally:
        dist.destroy_process_group()


def test_two_ranks_cast_the_same_rays_without_a_collective(tmp_path):
    import torch.multiprocessing as mp
    from tests.test_cols_host import _free_port
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    got = [np.load(tmp_path / f'rank{q}.npz') for q in range(2)]
    assert got[0]['built_with'] == 0 and got[1]['built_with'] == 0
    np.testing.assert_array_equal(got[0]['indices'], got[1]['indices'])
    np.testing.assert_array_equal(got[0]['Theta'], got[1]['Theta'])       # all-reduced partial products: the same on both
    eng, grid = OracleRaycastEngine(), camera_grid()
    whole = SPR(field_of_rank(grid), 2, None, engine=eng)
    whole.fit(select_modes='number', n_modes=4)
    whole.train(notebook_camera().project(grid, feature=1, n_features=2, to_host=False, engine=eng))
    sign = np.sign(np.sum(whole.Theta * got[0]['Theta'], axis=0))          # a mode's sign is free
    assert np.allclose(got[0]['Theta'] * sign, whole.Theta, rtol=0, atol=1e-10 * np.abs(whole.Theta).max())
