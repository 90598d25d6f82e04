"""RectilinearGrid on the CPU: the class, the brute-force oracle for stored edges that tests/test_raycast_rect_gpu.py holds
the rectilinear kernels of csrc/raycast.hip to, the host wiring of camera.project / Resampler / resample_to_grid, and the
condition on the cases the GPU file casts.

Oracle: every cell against every segment, the slab test of tests/test_raycast_host in np.longdouble on the same float64
edges and end points; no traversal, no bisection, no code shared with csrc/raycast.hip.  Its records have the format of
tests.test_raycast_host.oracle_segments (cells, chords, length, clipped, cross, d), so chord_bar, margin, coordinate_scale
and oracle_csr(..., recs=recs) of that file apply as they are.

The cases (grids, segments, cameras) live here and are imported by the GPU file; the records of a case are computed once."""
import functools
import pickle

import numpy as np
import pytest
import torch

from openmeasure_amd.sparse_sensing import DeviceCSR
from openmeasure_amd.utils import RectilinearGrid, Resampler, VoxelGrid, resample_to_grid
from tests.numpy_engine import NumpyEngine
from tests.test_raycast_gpu import hand_segments
from tests.test_raycast_host import (LD, _slab, camera_grid, coordinate_scale, focused_camera, margin, notebook_camera,
                                     oracle_csr, oracle_segments, pinhole_camera, segments_of)


# ------------------------------------------------------------------------------------------------ the oracle
def edge_oracle_segments(seg, grid):
    """seg (n, 6) float64 -> one record per segment, as tests.test_raycast_host.oracle_segments gives them, for a grid
    with stored edges: ALL cells x all segments (the grids are tiny)"""
    ex, ey, ez = (np.asarray(e, dtype=LD) for e in grid.edges)
    nx, ny, nz = grid.dims
    k, j, i = (v.ravel() for v in np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing='ij'))
    ids = (i + nx * (j + ny * k)).astype(np.int64)            # ascending: i fastest
    lo = np.stack([ex[i], ey[j], ez[k]], axis=1)
    hi = np.stack([ex[i + 1], ey[j + 1], ez[k + 1]], axis=1)
    glo, ghi = np.array([[ex[0], ey[0], ez[0]]], dtype=LD), np.array([[ex[-1], ey[-1], ez[-1]]], dtype=LD)
    out = []
    for s in np.asarray(seg, dtype=np.float64):
        a, d = s[:3].astype(LD), s[3:].astype(LD) - s[:3].astype(LD)
        L = np.sqrt(np.sum(d * d))
        if L == 0:
            out.append(dict(cells=np.zeros(0, dtype=np.int64), chords=np.zeros(0, dtype=LD), length=L, clipped=LD(0), cross=[],
                            d=d))
            continue

        def clip(blo, bhi):
            te, tx = np.zeros(len(blo), dtype=LD), np.ones(len(blo), dtype=LD)
            for ax in range(3):
                e, x = _slab(a[ax], d[ax], blo[:, ax], bhi[:, ax])
                te, tx = np.maximum(te, e), np.minimum(tx, x)
            return te, tx

        te, tx = clip(lo, hi)
        hit = np.flatnonzero(tx > te)
        g0, g1 = clip(glo, ghi)
        clipped = (g1[0] - g0[0]) * L if g1[0] > g0[0] else LD(0)
        cross = []
        if clipped > 0:
            for ax, planes in enumerate((ex, ey, ez)):
                c0, c1 = sorted((a[ax] + g0[0] * d[ax], a[ax] + g1[0] * d[ax]))
                slack = LD(1e-12) * max(abs(c0), abs(c1), 1e-300)
                if d[ax] != 0 and np.any((planes >= c0 - slack) & (planes <= c1 + slack)):
                    cross.append(ax)
        out.append(dict(cells=ids[hit], chords=((tx - te) * L)[hit], length=L, clipped=clipped, cross=cross, d=d))
    return out


class OracleRectEngine(NumpyEngine):
    """NumpyEngine whose raycast is the edge oracle, with the contract of HipEngine.raycast; counts its calls"""

    def __init__(self):
        super().__init__()
        self.raycast_calls = 0

    def raycast(self, segments, grid, n_ray, weights='hit', col0=0):
        assert isinstance(grid, RectilinearGrid)
        assert isinstance(segments, np.ndarray) and segments.dtype == np.float64 and segments.shape[1] == 6
        assert segments.shape[0] % n_ray == 0 and np.all(np.isfinite(segments)) and weights in ('hit', 'length')
        self.raycast_calls += 1
        indptr, indices, vals, _ = oracle_csr(segments, grid, n_ray, weights, col0, recs=edge_oracle_segments(segments, grid))
        return torch.from_numpy(indptr), torch.from_numpy(indices), torch.from_numpy(vals)


# ------------------------------------------------------------------------------------------------ shared cases
def _geometric(k, ratio=1.6):
    """c_k = sum_{i < k} ratio^i"""
    return float(sum(ratio ** i for i in range(k)))


def hand_grids():
    """the three grids of the issue over the box of HAND_GRID: x -1.1 .. 1.4, y 0.3 .. 1.3, z -0.4 .. 2.6"""
    graded_x = [-1.1 + 2.5 * _geometric(k) / _geometric(9) for k in range(10)]
    graded_z = [-0.4 + 3.0 * (1.0 - _geometric(7 - k) / _geometric(7)) for k in range(8)]
    return {'stretched': RectilinearGrid([-1.1, -0.85, -0.45, 0.2, 0.55, 1.4], [0.3, 0.4, 0.6, 0.9, 1.3], [-0.4, 0.1, 1.7, 2.6]),
            'graded': RectilinearGrid(graded_x, [0.3, 1.3], graded_z),          # ONE cell along y: the shortest bisection
            'sliver': RectilinearGrid([-1.1, -0.1, -0.099, 0.3, 1.4], [0.3, 0.8, 0.8005, 1.3], [-0.4, 1.0, 1.001, 2.6])}


HAND_NAMES = ('stretched', 'graded', 'sliver')
HAND_DIMS = {'stretched': (5, 4, 3), 'graded': (9, 1, 7), 'sliver': (4, 3, 3)}


@functools.lru_cache(maxsize=None)
def hand_records(name):
    """(grid, the 257 segments, their records): computed once; a prefix of the segments has the prefix of the records"""
    grid = hand_grids()[name]
    seg = hand_segments()
    return grid, seg, edge_oracle_segments(seg, grid)


def graded_edges(lo, hi, n, ratio):
    """n cells between lo and hi whose widths grow by `ratio` from one to the next; the two ends are lo and hi exactly"""
    w = ratio ** np.arange(n)
    e = lo + (hi - lo) * np.concatenate([[0.0], np.cumsum(w)]) / w.sum()
    e[0], e[-1] = lo, hi
    return e


def stretched_camera_grid():
    """8 x 6 x 5 cells over the box of camera_grid() -- the same corner coordinates -- with interior edges graded by 1.3
    (x and z refined towards their low ends, y towards its high end)"""
    (x0, y0, z0), (x1, y1, z1) = camera_grid().corners()
    return RectilinearGrid(graded_edges(x0, x1, 8, 1.3), graded_edges(y0, y1, 6, 1 / 1.3), graded_edges(z0, z1, 5, 1.3))


CAMERA_CASES = ('notebook', 'tilted', 'pinhole', 'thin_lens')


def camera_case(case):
    return {'notebook': (notebook_camera(), 'parallel'), 'tilted': (notebook_camera((0.09, 0.05, 0.12)), 'parallel'),
            'pinhole': (pinhole_camera(), 'pinhole'), 'thin_lens': (focused_camera(), 'thin_lens')}[case]


@functools.lru_cache(maxsize=None)
def camera_records(case):
    """(grid, segments, n_ray, records) of one camera through stretched_camera_grid()"""
    cam, type_rec = camera_case(case)
    grid = stretched_camera_grid()
    seg, n_ray = segments_of(cam, type_rec)
    return grid, seg, n_ray, edge_oracle_segments(seg, grid)


DYADIC = dict(origin=(-1.0, 0.25, -0.5), spacing=(0.5, 0.25, 1.0), dims=(5, 4, 3))   # origin + k * spacing is exact


def dyadic_segments():
    """257 segments for the DYADIC grid: the six axis directions through the centre of cell (2, 1, 1), one oblique segment
    per octant, random ones.  (hand_segments() is not used with this grid: its segment 14 passes within 1e-16 of a cell
    edge of DYADIC, which the margin condition rules out.)"""
    cx, cy, cz = 0.25, 0.625, 1.0
    seg = [[-2.0, cy, cz, 2.5, cy, cz], [2.5, cy, cz, -2.0, cy, cz], [cx, -1.0, cz, cx, 2.0, cz], [cx, 2.0, cz, cx, -1.0, cz],
           [cx, cy, -1.5, cx, cy, 3.5], [cx, cy, 3.5, cx, cy, -1.5]]
    p0 = np.array([0.21, 0.71, 1.23])
    for sx in (1, -1):
        for sy in (1, -1):
            for sz in (1, -1):
                v = np.array([sx * 0.9, sy * 0.45, sz * 1.1])
                seg.append([*(p0 - 1.7 * v), *(p0 + 1.9 * v)])
    rnd = np.random.default_rng(7).uniform([-1.7, -0.2, -1.3], [2.2, 1.7, 3.3], size=(257 - len(seg), 2, 3)).reshape(-1, 6)
    return np.concatenate([np.array(seg), rnd])


# ------------------------------------------------------------------------------------------------ the class
def test_refusals():
    ok = [0.0, 1.0, 2.5]
    for bad in ([0.0], [], [[0.0, 1.0], [2.0, 3.0]]):                          # fewer than two entries, not 1-D
        with pytest.raises(ValueError, match='at least two'):
            RectilinearGrid(bad, ok, ok)
    for bad in ([0.0, np.nan, 2.0], [0.0, 1.0, np.inf], [-np.inf, 0.0]):
        with pytest.raises(ValueError, match='finite'):
            RectilinearGrid(ok, bad, ok)
    for bad in ([0.0, 1.0, 1.0], [0.0, 2.0, 1.0], [1.0, 0.0]):
        with pytest.raises(ValueError, match='ascending'):
            RectilinearGrid(ok, ok, bad)
    xr, yr, zr = np.array([0.0, 1.0, 3.0]), np.array([0.0, 0.5, 0.75, 2.0]), np.array([-1.0, 0.0])
    with pytest.raises(ValueError, match='indexing'):
        RectilinearGrid.from_axes(*np.meshgrid(xr, yr, zr, indexing='xy'))
    with pytest.raises(ValueError, match='at least two'):
        RectilinearGrid.from_axes(xr, yr, np.array([1.0]))
    with pytest.raises(NotImplementedError, match='cells below 2\\^31'):
        RectilinearGrid(np.arange(2049.0), np.arange(1025.0), np.arange(1025.0))
    big = RectilinearGrid(np.arange(2048.0), np.arange(1025.0), np.arange(1025.0))   # 2047 * 2^20 cells: below the cap
    assert big.n_cells == 2047 * 1024 * 1024 < 2 ** 31


def test_from_axes_reads_lines_and_ij_meshgrids():
    xr, yr, zr = np.array([0.0, 1.0, 3.0]), np.array([0.0, 0.5, 0.75, 2.0]), np.array([-1.0, 0.0])
    g = RectilinearGrid.from_axes(xr, yr, zr)
    assert g.dims == (2, 3, 1) and g.n_cells == 6
    assert all(np.array_equal(e, a) and e.dtype == np.float64 and e.flags.c_contiguous for e, a in zip(g.edges, (xr, yr, zr)))
    g3 = RectilinearGrid.from_axes(*np.meshgrid(xr, yr, zr, indexing='ij'))
    assert g3.dims == g.dims and all(np.array_equal(p, q) for p, q in zip(g3.edges, g.edges))
    assert np.array_equal(g.corners(), [[0.0, 0.0, -1.0], [3.0, 2.0, 0.0]])
    f32 = RectilinearGrid.from_axes(xr.astype(np.float32), list(yr), tuple(zr))        # any array-like, widened
    assert all(np.array_equal(p, q) for p, q in zip(f32.edges, g.edges))
    xr[1] = 2.0                                                                        # the grid holds copies
    assert g.edges[0][1] == 1.0
    # the uniform classes keep refusing what this one takes
    with pytest.raises(ValueError, match='uniform'):
        VoxelGrid.from_axes(g.edges[0], np.array([0.0, 1.0]), zr)
    with pytest.raises(ValueError, match='uniform'):
        resample_to_grid(np.zeros((4, 3)), np.zeros((4, 1)), [g.edges[0], np.array([0.0, 1.0]), zr])


def test_centres_ids_and_volumes():
    g = hand_grids()['stretched']
    assert g.dims == (5, 4, 3) and g.n_cells == 60
    xyz, vol = g.cell_centers(), g.cell_volumes()
    assert xyz.shape == (60, 3) and vol.shape == (60,)
    ex, ey, ez = g.edges
    for cid, (i, j, k) in ((0, (0, 0, 0)), (1, (1, 0, 0)), (5, (0, 1, 0)), (20, (0, 0, 1)), (59, (4, 3, 2)), (33, (3, 2, 1))):
        assert cid == i + 5 * (j + 4 * k)
        assert np.array_equal(xyz[cid], [0.5 * (ex[i] + ex[i + 1]), 0.5 * (ey[j] + ey[j + 1]), 0.5 * (ez[k] + ez[k + 1])])
        assert vol[cid] == pytest.approx((ex[i + 1] - ex[i]) * (ey[j + 1] - ey[j]) * (ez[k + 1] - ez[k]), rel=1e-15)
    for name, grid in hand_grids().items():
        assert grid.dims == HAND_DIMS[name]
        assert np.allclose(grid.corners(), [[-1.1, 0.3, -0.4], [1.4, 1.3, 2.6]], rtol=0, atol=1e-15), name
        assert grid.cell_volumes().sum() == pytest.approx(2.5 * 1.0 * 3.0, rel=1e-14) and np.all(grid.cell_volumes() > 0)
    graded = hand_grids()['graded']
    wx, wz = np.diff(graded.edges[0]), np.diff(graded.edges[2])
    assert wx.max() / wx.min() == pytest.approx(1.6 ** 8) and np.all(np.diff(wz) < 0)   # about 43; z graded the other way


def test_from_voxel_grid_has_the_cells_of_the_voxel_grid():
    for v in (VoxelGrid(**DYADIC), VoxelGrid((-1.1, 0.3, -0.4), (0.5, 0.25, 1.0), (5, 4, 3)), camera_grid()):
        g = RectilinearGrid.from_voxel_grid(v)
        assert g.dims == v.dims and g.n_cells == v.n_cells
        scale = np.abs(v.corners()).max()
        assert np.allclose(g.cell_centers(), v.cell_centers(), rtol=0, atol=4 * 2.0 ** -52 * scale)   # the same order of ids
        assert np.allclose(g.corners(), v.corners(), rtol=0, atol=2 * 2.0 ** -52 * scale)
        assert np.allclose(g.cell_volumes(), np.prod(v.spacing), rtol=1e-13)
    g = RectilinearGrid.from_voxel_grid(VoxelGrid(**DYADIC))
    assert np.array_equal(g.edges[0], [-1.0, -0.5, 0.0, 0.5, 1.0, 1.5]) and np.array_equal(g.edges[2], [-0.5, 0.5, 1.5, 2.5])


def test_pickles_as_host_arrays_without_the_device_cache():
    g = hand_grids()['sliver']
    g._device_edges = ('an engine', ('three', 'device', 'tensors'))                   # what HipEngine leaves on the object
    r = pickle.loads(pickle.dumps(g))
    assert isinstance(r, RectilinearGrid) and r.dims == g.dims and r._device_edges is None
    assert all(isinstance(e, np.ndarray) and np.array_equal(e, f) for e, f in zip(r.edges, g.edges))
    assert b'device' not in pickle.dumps(g)


# ------------------------------------------------------------------------------------------------ the oracle itself
def test_edge_oracle_on_cases_known_by_hand():
    grid = RectilinearGrid([0.0, 1.0, 1.5, 4.0], [0.0, 2.0, 4.0], [0.0, 3.0, 6.0])     # x cells of width 1, 0.5, 2.5
    seg = np.array([[-1.0, 1.0, 1.5, 5.0, 1.0, 1.5],          # along +x through cells 0, 1, 2 of the first row
                    [0.5, 1.0, 1.5, 2.5, 1.0, 1.5],           # inside -> inside: half a cell, a whole one, 1 of 2.5
                    [0.5, 5.0, 1.5, 2.5, 5.0, 1.5],           # outside the y slab
                    [0.5, 0.5, 0.5, 0.5, 0.5, 0.5],           # a == b
                    [1.25, 3.0, -1.0, 1.25, 3.0, 7.0],        # along +z through cell (1, 1, 0) and (1, 1, 1)
                    [1.0, 1.0, 1.0, 1.0, 1.0, 2.0]])          # in the plane x = 1: touches two cells, inside none
    r = edge_oracle_segments(seg, grid)
    assert r[0]['cells'].tolist() == [0, 1, 2] and np.allclose(r[0]['chords'].astype(float), [1.0, 0.5, 2.5])
    assert r[1]['cells'].tolist() == [0, 1, 2] and np.allclose(r[1]['chords'].astype(float), [0.5, 0.5, 1.0])
    assert r[0]['cross'] == [0] and float(r[0]['clipped']) == 4.0 and float(r[0]['length']) == 6.0
    assert len(r[2]['cells']) == 0 and len(r[3]['cells']) == 0 and len(r[5]['cells']) == 0
    assert r[4]['cells'].tolist() == [1 + 3 * 1, 1 + 3 * (1 + 2 * 1)] and np.allclose(r[4]['chords'].astype(float), 3.0)
    diag = edge_oracle_segments(np.array([[0.25, 0.5, 0.75, 3.75, 3.5, 5.25]]), grid)[0]
    assert abs(float(diag['chords'].sum() - diag['clipped'])) < 1e-15 and diag['cross'] == [0, 1, 2]
    assert abs(float(diag['clipped'] - diag['length'])) < 1e-15                        # it lies inside the grid
    ip, ix, v, _ = oracle_csr(seg[[0, 1]], grid, 2, 'length', col0=12, recs=r[:2])
    assert ip.tolist() == [0, 3] and ix.tolist() == [12, 13, 14] and np.allclose(v, [0.75, 0.5, 1.75])


def test_edge_oracle_agrees_with_the_uniform_oracle_on_a_dyadic_grid():
    """origin + k * spacing is exact here, so both oracles see the same boxes: the same cells, chords to longdouble rounding"""
    v = VoxelGrid(**DYADIC)
    g = RectilinearGrid.from_voxel_grid(v)
    seg = np.concatenate([hand_segments(), dyadic_segments()])
    uni, rect = oracle_segments(seg, v), edge_oracle_segments(seg, g)
    assert sum(len(r['cells']) for r in uni) > 500
    eps_ld = float(np.finfo(LD).eps)
    for u, r in zip(uni, rect):
        assert np.array_equal(u['cells'], r['cells']) and u['cross'] == r['cross']
        assert float(abs(u['clipped'] - r['clipped'])) <= 8 * eps_ld * float(u['length'])
        if len(u['cells']):
            assert float(np.max(np.abs(u['chords'] - r['chords']))) <= 8 * eps_ld * float(u['length'])


# ------------------------------------------------------------------------------------------------ the condition on the GPU cases
@pytest.mark.parametrize('name', HAND_NAMES)
def test_the_hand_cases_stay_clear_of_grazing_rays(name):
    """hits / most cells per segment / margin as the issue records them: 853 / 10, 977 / 15, 789 / 8, margin 9.36e-6 S"""
    grid, seg, recs = hand_records(name)
    assert len(seg) == 257
    S = coordinate_scale(seg, grid)
    hits, most = sum(len(r['cells']) for r in recs), max(len(r['cells']) for r in recs)
    print(f'{name}: {hits} hits, at most {most} cells per segment, margin {margin(recs, S):.3e} S')
    assert (hits, most) == {'stretched': (853, 10), 'graded': (977, 15), 'sliver': (789, 8)}[name]
    assert most <= sum(grid.dims) + 2
    assert margin(recs, S) >= 1e-9
    for n_seg in (1, 63, 65):                                  # every prefix the GPU file casts
        assert margin(recs[:n_seg], coordinate_scale(seg[:n_seg], grid)) >= 1e-9
    empty = [s for s, r in enumerate(recs[:20]) if not len(r['cells'])]
    assert empty == [17, 18, 19]                               # the miss, the segment outside its slab, a == b


@pytest.mark.parametrize('case', CAMERA_CASES)
def test_the_camera_cases_stay_clear_of_grazing_rays(case):
    grid, seg, n_ray, recs = camera_records(case)
    assert n_ray == (1 if case in ('notebook', 'tilted') else 3) and len(seg) == 64 * n_ray
    assert np.array_equal(grid.corners(), camera_grid().corners()) and grid.dims == camera_grid().dims
    w = [np.diff(e) for e in grid.edges]
    assert all(np.allclose(x[1:] / x[:-1], x[1] / x[0], rtol=1e-9) for x in w)         # graded: a constant ratio of widths
    assert sum(len(r['cells']) for r in recs) > 0
    m = margin(recs, coordinate_scale(seg, grid))
    print(f'camera {case}: {sum(len(r["cells"]) for r in recs)} hits, margin {m:.3e} S')
    assert m >= 1e-9


def test_dyadic_agreement_case_stays_clear_of_grazing_rays():
    seg = dyadic_segments()
    g = RectilinearGrid.from_voxel_grid(VoxelGrid(**DYADIC))
    recs = edge_oracle_segments(seg, g)
    assert len(seg) == 257 and sum(len(r['cells']) for r in recs) > 500
    assert margin(recs, coordinate_scale(seg, g)) >= 1e-9


# ------------------------------------------------------------------------------------------------ host wiring
def test_project_takes_a_rectilinear_grid():
    import scipy.sparse as sp
    eng, grid, cam = OracleRectEngine(), stretched_camera_grid(), notebook_camera()
    C = cam.project(grid, engine=eng)
    assert sp.issparse(C) and C.format == 'csr' and C.shape == (64, 240) and eng.raycast_calls == 1
    # the 6 x 5 pixels whose centres lie in the box look along x through the 8 cells of one row; the others see nothing
    assert C.nnz == 30 * 8 and set(np.diff(C.indptr).tolist()) == {0, 8} and np.all(C.data == 1.0)
    ey, ez = grid.edges[1], grid.edges[2]
    centres = (cam._sensor_coordinates() @ np.linalg.inv(cam._extr_matrix()).T)[:, :3]
    for p in np.flatnonzero(np.diff(C.indptr)):
        cols = C.indices[C.indptr[p]:C.indptr[p + 1]]
        j, k = np.searchsorted(ey, centres[p, 1]) - 1, np.searchsorted(ez, centres[p, 2]) - 1
        assert cols.tolist() == [i + 8 * (j + 6 * k) for i in range(8)]
    D = cam.project(grid, feature=1, n_features=2, to_host=False, engine=eng)
    assert isinstance(D, DeviceCSR) and D.shape == (64, 480) and D.nnz == C.nnz and eng.raycast_calls == 2
    H = D.tocsr()
    assert np.array_equal(H.indptr, C.indptr) and np.array_equal(H.indices, C.indices + 240) and np.array_equal(H.data, C.data)
    W = cam.project(grid, weights='length', engine=eng)
    assert np.array_equal(W.indices, C.indices)
    assert np.allclose(W.data.reshape(30, 8), np.diff(grid.edges[0])[None, :], rtol=1e-12)      # chords = the x widths
    P = cam.project(grid, 'pinhole', N_rand=3, seed=2, engine=eng)
    assert P.shape == (64, 240) and P.nnz > 0
    for bad in (object(), grid.edges, None):
        with pytest.raises(TypeError):
            cam.project(bad, engine=eng)
    with pytest.raises(ValueError, match='weights'):
        cam.project(grid, weights='area', engine=eng)
    assert eng.raycast_calls == 4


def test_resampler_takes_the_centres_of_a_rectilinear_grid():
    from tests.test_resample_host import OracleResampleEngine
    grid = hand_grids()['stretched']
    rng = np.random.default_rng(4)
    src = rng.uniform(grid.corners()[0] - 0.2, grid.corners()[1] + 0.2, size=(300, 3))
    X = rng.standard_normal((2 * 300, 5))
    for method, k in (('nearest', 1), ('idw', 4)):
        eng = OracleResampleEngine()
        a = Resampler(src, grid, method=method, k=k, engine=eng)
        b = Resampler(src, grid.cell_centers(), method=method, k=k, engine=eng)
        assert a.n_dst == grid.n_cells == 60 and a.index.shape == (60, k)
        for p, q in zip(a.tensors(), b.tensors()):
            assert np.asarray(p).tobytes() == np.asarray(q).tobytes()
        out = resample_to_grid(src, X, grid, method=method, k=k, engine=eng)
        assert out[0] is grid and np.array_equal(out[2], grid.cell_centers())
        assert np.array_equal(out[1], a.apply(X, 2))
