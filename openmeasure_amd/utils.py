"""Tomography front end with the surface of ``openmeasure.utils`` (reference: src/openmeasure/utils.py).

A camera image of a volumetric field f is p = C f (docs/ctc_doc.ipynb).  The reference builds C in a Python loop with one
pyvista line query per pixel and per random ray (``camera.project``, utils.py:318-469).  Here the end points of all rays are
formed at once on the host (``camera.segments``, a vectorised restatement of the reference's arithmetic) and cast through
a uniform or a rectilinear voxel grid on the device (csrc/raycast.hip): segments in, CSR out.  ``project(to_host=False)``
returns a ``DeviceCSR`` that ``SPR.train`` takes as it is.

What differs from the reference, by design:
  * the mesh is a ``VoxelGrid`` (origin, spacing, dims) or a ``RectilinearGrid`` (three arrays of ascending edge
    coordinates: a stretched structured grid), not a pyvista object; curvilinear and unstructured meshes are outside this
    module;
  * a cell belongs to a ray iff the ray has positive length inside it in the kernel's float64 arithmetic.  VTK's locator
    decides rays that graze a face, an edge or a corner by its own tolerance; agreement on such rays is not pinned;
  * the random rays come from ONE ``np.random.default_rng(seed)``, so a projection can be repeated (the reference makes an
    unseeded generator per pixel);
  * ``weights='length'`` gives the line integral (mean chord length over the pixel's rays), which the reference does not form;
  * an unknown ``type_rec`` is a ``ValueError`` (the reference silently returns an empty C);
  * ``generate_camera`` returns a pyvista object and raises ``NotImplementedError``.

The step before ``project`` in the reference's notebook is ``resample_to_grid`` (utils.py:17-99): a solution on an unstructured
mesh is brought onto the uniform grid.  Here a mesh is its (n_cells, 3) cell centres, and ``Resampler`` maps values at one such
cloud to another cloud or to the centres of a ``VoxelGrid`` or a ``RectilinearGrid`` on the device (csrc/resample.hip): a
neighbour search once per pair of meshes, then one pass over the snapshot matrix per application.  ``resample_to_grid(xyz, X, grid)`` returns the
reference's triple with the grid object in place of the pyvista mesh, and with a ``DeviceMatrix`` in, the chain
xyz, X -> X_int -> SPR(X_int, n_features, grid.cell_centers()) -> project -> train -> predict -> reconstruct never leaves HBM.
  * ``method='nearest'`` is ``scipy.interpolate.griddata(..., method='nearest')`` with ties decided by the lower source
    index; ``method='idw'`` is Shepard's inverse-distance weighting (power 2) over the k <= 8 nearest sources;
  * agreement with the reference's numbers is NOT pinned: VTK's probe filter interpolates inside the containing cell, on the
    connectivity of the mesh, which this package never sees.
"""
from __future__ import annotations

import numpy as np

from ._csr import DeviceCSR

__all__ = ['VoxelGrid', 'RectilinearGrid', 'camera', 'Resampler', 'resample_to_grid']


def _axis_lines(x, y, z):
    """Three 1-D float64 axes from 1-D arrays or from the three arrays of ``np.meshgrid(..., indexing='ij')``"""
    axes = []
    for d, a in enumerate((x, y, z)):
        a = np.asarray(a, dtype=np.float64)
        if a.ndim == 3:
            idx = [0, 0, 0]
            idx[d] = slice(None)
            line = a[tuple(idx)]
            shape = [1, 1, 1]
            shape[d] = -1
            if not np.array_equal(np.broadcast_to(line.reshape(shape), a.shape), a):
                raise ValueError("3-D coordinates must come from np.meshgrid(..., indexing='ij')")
            a = line
        if a.ndim != 1 or a.shape[0] < 2:
            raise ValueError('an axis needs at least two point coordinates')
        axes.append(a)
    return axes


class VoxelGrid:
    """A uniform grid of ``dims = (nx, ny, nz)`` axis-aligned cells: cell (i, j, k) is the box
    ``origin + (i, j, k) * spacing`` ... ``origin + (i + 1, j + 1, k + 1) * spacing`` and has the id ``i + nx (j + ny k)``.

    That is VTK's order of the cells of a structured grid, i fastest -- the order of ``pv.StructuredGrid(x, y, z)`` built
    from ``np.meshgrid(..., indexing='ij')`` as the reference's notebook does (cell 9) -- AS READ from VTK's documentation:
    it is not checked here against pyvista, which this package does not use."""

    def __init__(self, origin, spacing, dims):
        self.origin = np.asarray(origin, dtype=np.float64).reshape(-1)
        self.spacing = np.asarray(spacing, dtype=np.float64).reshape(-1)
        dims_in = np.asarray(dims).reshape(-1)
        if self.origin.shape != (3,) or self.spacing.shape != (3,) or dims_in.shape != (3,):
            raise ValueError('origin, spacing and dims have three entries each')
        if np.any(dims_in != np.floor(dims_in)) or np.any(dims_in < 1):
            raise ValueError('dims must be positive integers')
        self.dims = tuple(int(d) for d in dims_in)
        if not (np.all(np.isfinite(self.origin)) and np.all(np.isfinite(self.spacing)) and np.all(self.spacing > 0)):
            raise ValueError('origin and spacing must be finite, spacing positive')
        if self.n_cells >= 2 ** 31:
            raise NotImplementedError(f'{self.n_cells} cells: the ray caster numbers cells below 2^31')

    @property
    def n_cells(self):
        return self.dims[0] * self.dims[1] * self.dims[2]

    @classmethod
    def from_axes(cls, x, y, z):
        """The grid whose cell CORNERS are the given point coordinates, as ``pv.StructuredGrid(x, y, z)`` reads them: three
        1-D axes, or the three 3-D arrays of ``np.meshgrid(xr, yr, zr, indexing='ij')`` (notebook cell 9).  n points along an
        axis make n - 1 cells.  The spacing is (last - first) / (n - 1); a step that differs from it by more than 1e-5 of it
        is a ``ValueError`` (the notebook's ranges are float32, uniform to about 1e-6)."""
        axes = _axis_lines(x, y, z)
        origin, spacing = [], []
        for a in axes:
            h = (a[-1] - a[0]) / (a.shape[0] - 1)
            if not (np.isfinite(h) and h > 0) or np.max(np.abs(np.diff(a) - h)) > 1e-5 * h:
                raise ValueError('the point coordinates of an axis must ascend in uniform steps (1e-5 relative)')
            origin.append(a[0])
            spacing.append(h)
        return cls(origin, spacing, [a.shape[0] - 1 for a in axes])

    def cell_centers(self):
        """(n_cells, 3) centres in cell-id order: the ``xyz`` to hand to ``SPR``"""
        c = [self.origin[d] + (np.arange(self.dims[d]) + 0.5) * self.spacing[d] for d in range(3)]
        kk, jj, ii = np.meshgrid(c[2], c[1], c[0], indexing='ij')
        return np.stack([ii.ravel(), jj.ravel(), kk.ravel()], axis=1)

    def corners(self):
        """(2, 3): the lowest and the highest corner"""
        return np.stack([self.origin, self.origin + np.asarray(self.dims) * self.spacing])


class RectilinearGrid:
    """A tensor-product grid of ``dims = (nx, ny, nz)`` axis-aligned cells with arbitrary ascending edge coordinates: cell
    (i, j, k) is the box ``x_edges[i] .. x_edges[i + 1]`` x ``y_edges[j] .. y_edges[j + 1]`` x ``z_edges[k] .. z_edges[k + 1]``
    and has the id ``i + nx (j + ny k)``, the order of ``VoxelGrid``.  n + 1 edges along an axis make n >= 1 cells.  This is
    ``pv.StructuredGrid(x, y, z)`` of three stretched axes: the structured CFD grid that is refined towards a burner or a wall.

    ``camera.project`` casts through it with the rectilinear kernels of csrc/raycast.hip (the planes are the stored edges,
    the start cell is found by bisection); ``Resampler`` and ``resample_to_grid`` take it as a target.  The object pickles as
    its three host arrays; the device copy of the edges that an engine makes at the first cast is a cache and is not pickled."""

    def __init__(self, x_edges, y_edges, z_edges):
        edges = []
        for name, e in zip('xyz', (x_edges, y_edges, z_edges)):
            e = np.array(e, dtype=np.float64, order='C')          # a contiguous copy
            if e.ndim != 1 or e.shape[0] < 2:
                raise ValueError(f'{name}_edges: an axis needs at least two edge coordinates in a 1-D array')
            if not np.all(np.isfinite(e)):
                raise ValueError(f'{name}_edges must be finite')
            if not np.all(np.diff(e) > 0):
                raise ValueError(f'{name}_edges must be strictly ascending')
            edges.append(e)
        self.edges = tuple(edges)
        self.dims = tuple(int(e.shape[0]) - 1 for e in edges)
        self._device_edges = None                                 # (engine, tensors): HipEngine's cache
        if self.n_cells >= 2 ** 31:
            raise NotImplementedError(f'{self.n_cells} cells: the ray caster numbers cells below 2^31')

    @property
    def n_cells(self):
        return self.dims[0] * self.dims[1] * self.dims[2]

    @classmethod
    def from_axes(cls, x, y, z):
        """The grid whose cell CORNERS are the given point coordinates: three 1-D axes, or the three 3-D arrays of
        ``np.meshgrid(xr, yr, zr, indexing='ij')``, read as ``VoxelGrid.from_axes`` reads them but with steps of any size."""
        return cls(*_axis_lines(x, y, z))

    @classmethod
    def from_voxel_grid(cls, grid):
        """The same cells as a ``VoxelGrid``: edges ``origin + arange(n + 1) * spacing``"""
        return cls(*(grid.origin[d] + np.arange(grid.dims[d] + 1) * grid.spacing[d] for d in range(3)))

    def cell_centers(self):
        """(n_cells, 3) centres ``0.5 * (e[i] + e[i + 1])`` in cell-id order: the ``xyz`` to hand to ``SPR``"""
        c = [0.5 * (e[:-1] + e[1:]) for e in self.edges]
        kk, jj, ii = np.meshgrid(c[2], c[1], c[0], indexing='ij')
        return np.stack([ii.ravel(), jj.ravel(), kk.ravel()], axis=1)

    def cell_volumes(self):
        """(n_cells,) volumes in cell-id order: the weights of any volume-weighted statistic on a stretched grid"""
        w = [np.diff(e) for e in self.edges]
        return (w[2][:, None, None] * w[1][None, :, None] * w[0][None, None, :]).ravel()

    def corners(self):
        """(2, 3): the lowest and the highest corner"""
        return np.array([[e[0] for e in self.edges], [e[-1] for e in self.edges]])

    def __reduce__(self):
        return (RectilinearGrid, self.edges)


class camera():
    """Reference :101-469.  Points and vectors are 4-D: x, y, z and 1 for points, 0 for vectors.

    Same constructor, attributes (``n_pixels``, ``sensor_size_m``, ``d``, ``m``, ``d_object``) and private helpers
    (``_extr_matrix``, ``_sensor_coordinates``) as the reference; ``project`` takes a ``VoxelGrid`` or a ``RectilinearGrid``."""

    TYPES = ('parallel', 'pinhole', 'thin_lens')

    def __init__(self, p_cam, theta, f_length, n_aper, d_sensor, sensor_size_px, px_size):
        self.p_cam = p_cam
        self.theta = theta
        self.f_length = f_length
        self.n_aper = n_aper
        self.d_sensor = d_sensor
        self.sensor_size_px = sensor_size_px
        self.px_size = px_size

        self.n_pixels = int(sensor_size_px[0] * sensor_size_px[1])
        self.sensor_size_m = px_size * sensor_size_px
        self.d = np.linalg.norm(p_cam - np.array([0, 0, 0, 1]))

        m = d_sensor / f_length - 1                           # :207-213
        if m > 1e-2:
            self.m = m
            self.d_object = f_length / (1 - f_length / d_sensor)
        else:
            self.m = 0
            self.d_object = -1

    def _extr_matrix(self):
        """The extrinsic camera matrix (:215-242)."""
        c, s = np.cos(self.theta), np.sin(self.theta)
        R_x = np.array([[1, 0, 0, 0], [0, c[0], -s[0], 0], [0, s[0], c[0], 0], [0, 0, 0, 1]])
        R_y = np.array([[c[1], 0, s[1], 0], [0, 1, 0, 0], [-s[1], 0, c[1], 0], [0, 0, 0, 1]])
        R_z = np.array([[c[2], -s[2], 0, 0], [s[2], c[2], 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
        E = np.linalg.multi_dot([R_x, R_y, R_z])
        T = -E @ self.p_cam
        E[:-1, -1] = T[:-1]
        return E

    def _sensor_coordinates(self):
        """The local pixel coordinates (:244-264), (n_pixels, 4), rows of the image one after the other from the top."""
        xs = np.linspace(-self.sensor_size_m[0] / 2 + self.px_size / 2, self.sensor_size_m[0] / 2 - self.px_size / 2,
                         self.sensor_size_px[0])
        ys = np.linspace(self.sensor_size_m[1] / 2 - self.px_size / 2, -self.sensor_size_m[1] / 2 + self.px_size / 2,
                         self.sensor_size_px[1])
        xs_grid, ys_grid = np.meshgrid(xs, ys)
        xyz_sl = np.zeros((xs_grid.size, 4))
        xyz_sl[:, 0] = xs_grid.flatten()
        xyz_sl[:, 1] = ys_grid.flatten()
        xyz_sl[:, 3] = 1.
        return xyz_sl

    def generate_camera(self):
        """Reference :287-316 returns a pyvista object for plotting."""
        raise NotImplementedError('generate_camera builds a pyvista object (reference utils.py:287-316) and is not part of '
                                  'this implementation.')

    # ------------------------------------------------------------------ rays
    def segments(self, type_rec='parallel', N_rand=10, seed=None, draws=None):
        """End points ``(a, b)``, each ``(n_pixels, n_ray, 3)`` in global coordinates, of the line queries the reference
        makes for every pixel (the two arguments of ``find_cells_intersecting_line``, :372, :406, :454):

        'parallel'   n_ray = 1 (``N_rand`` is ignored): from the pixel centre along the optical axis to depth 2 d;
        'pinhole'    n_ray = N_rand: from a uniformly jittered point of the pixel through the lens centre, length 2 d;
        'thin_lens'  n_ray = N_rand: from a random point of the lens towards the image of the jittered pixel point on the
                     object plane, length 2 d.  As in the reference (:439) every ray of pixel i starts at lens point i: the
                     reference draws n_pixels * N_rand lens points and reads only the first n_pixels of them, one per
                     pixel, not one per ray.  That is restated literally.  ``m == 0`` (focus at infinity) is the
                     reference's ``ValueError``.

        The uniform numbers in [0, 1) come from one ``np.random.default_rng(seed)``, or are passed in as
        ``draws = {'jitter': (n_pixels, N_rand, 2), 'lens': (n_pixels, 2)}``: jitter[..., 0] / [..., 1] move the point by
        ``px_size (u - 0.5)`` in x / y, lens[:, 0] / [:, 1] give the radius ``R sqrt(u)`` and the angle ``2 pi u``.
        An unknown ``type_rec`` raises a ``ValueError``; the reference silently returns an empty C."""
        if type_rec not in self.TYPES:
            raise ValueError(f'type_rec must be one of {self.TYPES}, got {type_rec!r}')
        if type_rec == 'thin_lens' and self.m == 0:
            raise ValueError('For focus at infinity use a different model')   # :421-422
        E_inv = np.linalg.inv(self._extr_matrix())
        xyz_sl = self._sensor_coordinates()
        n_pix = self.n_pixels

        def to_global(pl):                                    # (..., 4) local points -> (..., 3) global
            return (pl @ E_inv.T)[..., :3]

        if type_rec == 'parallel':                            # :358-372
            far = xyz_sl.copy()
            far[:, 2] = -2 * self.d
            return to_global(xyz_sl)[:, None, :], to_global(far)[:, None, :]

        N_rand = int(N_rand)
        if N_rand < 1:
            raise ValueError('N_rand must be at least 1')
        if draws is None:
            rng = np.random.default_rng(seed)
            draws = {'lens': rng.random((2, n_pix * N_rand))[:, :n_pix].T, 'jitter': rng.random((n_pix, N_rand, 2))}
        jitter = np.asarray(draws['jitter'], dtype=np.float64)
        if jitter.shape != (n_pix, N_rand, 2):
            raise ValueError(f"draws['jitter'] must be {(n_pix, N_rand, 2)}, got {jitter.shape}")
        psl = np.zeros((n_pix, N_rand, 4))                    # the point on the sensor (:394-397, :434-437)
        psl[..., 0] = xyz_sl[:, None, 0] + self.px_size * (jitter[..., 0] - 0.5)
        psl[..., 1] = xyz_sl[:, None, 1] + self.px_size * (jitter[..., 1] - 0.5)
        psl[..., 3] = 1.

        if type_rec == 'pinhole':                             # :381-406
            pll = np.array([0, 0, -self.d_sensor, 1])
            v = pll - psl
            vfl = v / np.linalg.norm(v, axis=-1, keepdims=True)
            return to_global(psl), to_global(psl + 2 * self.d * vfl)

        lens = np.asarray(draws['lens'], dtype=np.float64)    # :266-285, :419-454
        if lens.shape != (n_pix, 2):
            raise ValueError(f"draws['lens'] must be {(n_pix, 2)}, got {lens.shape}")
        R = self.f_length / (self.n_aper * 2)
        r = R * np.sqrt(lens[:, 0])
        ang = lens[:, 1] * 2 * np.pi
        pll = np.zeros((n_pix, 1, 4))
        pll[:, 0, 0] = r * np.cos(ang)
        pll[:, 0, 1] = r * np.sin(ang)
        pll[:, 0, 2] = -self.d_sensor
        pll[:, 0, 3] = 1.
        pol = np.zeros_like(psl)                              # the point on the object plane
        pol[..., 0] = -psl[..., 0] / self.m
        pol[..., 1] = -psl[..., 1] / self.m
        pol[..., 2] = -(self.d_object + self.d_sensor)
        pol[..., 3] = 1.
        v = pol - pll
        vfl = v / np.linalg.norm(v, axis=-1, keepdims=True)
        pfl = pll + 2 * self.d * vfl
        return to_global(np.broadcast_to(pll, pfl.shape)), to_global(pfl)

    # ------------------------------------------------------------------ C
    def project(self, grid, type_rec='parallel', N_rand=10, verbose=False, *, seed=None, weights='hit', feature=None,
                n_features=1, to_host=True, engine=None):
        """The matrix C of the projection p = C f (reference :318-469) for a ``VoxelGrid`` or a ``RectilinearGrid``.

        Returns a ``scipy.sparse.csr_matrix`` of shape ``(n_pixels, n_cells)`` as the reference does, or with
        ``to_host=False`` a ``DeviceCSR`` whose arrays stay in HBM.  ``weights='hit'``: 1 for every cell that any ray of
        the pixel crosses (the reference's C); ``weights='length'``: the chord lengths inside the cell, summed over the
        pixel's rays and divided by their number.  ``feature`` / ``n_features`` place the columns in the block of one
        feature of a feature-major snapshot matrix, shape ``(n_pixels, n_features * n_cells)`` -- what the notebook's cell
        14 does by hand.  ``seed``: see ``segments``.  ``engine``: the engine to cast with (default: a ``HipEngine``)."""
        if not isinstance(grid, (VoxelGrid, RectilinearGrid)):
            raise TypeError('project takes a VoxelGrid or a RectilinearGrid (pyvista meshes are outside this implementation)')
        if weights not in ('hit', 'length'):
            raise ValueError("weights must be 'hit' or 'length'")
        n_features = int(n_features)
        f = 0 if feature is None else int(feature)
        if n_features < 1 or not 0 <= f < n_features:
            raise ValueError(f'feature {feature} is outside the {n_features} feature blocks')
        a, b = self.segments(type_rec, N_rand, seed=seed)
        n_ray = a.shape[1]
        seg = np.concatenate([a, b], axis=2).reshape(-1, 6)
        if not np.all(np.isfinite(seg)):
            raise ValueError('the rays of this camera have end points that are not finite')
        if engine is None:
            from .engine import HipEngine
            engine = HipEngine()
        if verbose:
            print(f'Casting {seg.shape[0]} rays of {self.n_pixels} pixels through {grid.n_cells} cells', flush=True)
        indptr, indices, vals = engine.raycast(seg, grid, n_ray, weights, f * grid.n_cells)
        C = DeviceCSR(indptr, indices, vals, (self.n_pixels, n_features * grid.n_cells), engine=engine)
        return C.tocsr() if to_host else C


# ---------------------------------------------------------------------- resampling
def _cloud(xyz, what):
    """(n, 3) float64 host array of finite coordinates, below 2^31 points; the size is checked before anything is copied"""
    shape = np.shape(xyz)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f'{what} must be an (n, 3) array of cell centres, got shape {shape}')
    if shape[0] == 0:
        raise ValueError(f'{what} holds no points')
    if shape[0] >= 2 ** 31:
        raise NotImplementedError(f'{what} holds {shape[0]} points: the resampler numbers points below 2^31')
    a = np.ascontiguousarray(xyz, dtype=np.float64)
    if not np.all(np.isfinite(a)):
        raise ValueError(f'{what} has coordinates that are not finite')
    return a


def _refuse_sharded(*objs):
    from ._shard import RowShard
    for o in objs:
        if isinstance(o, RowShard) or isinstance(getattr(o, '_shard', None), RowShard):
            raise NotImplementedError('resampling a row-sharded matrix is outside this implementation: a resampled row '
                                      'depends on rows of other ranks')


class Resampler:
    """The sparse operator that carries values at the points ``xyz_src`` (n_src, 3) to the targets ``dst``: an (n_dst, 3)
    array, or a ``VoxelGrid``, which stands for its cell centres ``origin + (i + 0.5) * spacing`` in cell-id order (the
    kernel forms them itself, a 128^3 grid costs no coordinate array), or a ``RectilinearGrid``, whose ``cell_centers()`` are
    uploaded as an (n_dst, 3) array like any other cloud: sparing that array, 24 bytes per cell, is not worth a variant of the
    search kernel.  Built once per pair of meshes on the device (csrc/resample.hip), applied to any number of snapshot
    matrices with ``apply``.

    Neighbours of a target: the ``k`` sources smallest under (d2, source index), lexicographic, d2 the float64 squared
    distance of the float64 coordinates; equidistant sources are decided by the lower index and the lists are in that order.
    ``method='nearest'``: k = 1 (the argument ``k`` is not used), weight 1 -- ``scipy.interpolate.griddata(method='nearest')``.
    ``method='idw'``: ``k`` in 1 .. 8, Shepard's weights ``w_j = (1 / d2_j) / sum_i (1 / d2_i)`` (``power=2``; any other power
    is a ``ValueError``); a target that coincides with its first neighbour takes that value alone.
    ``max_distance=D``: a source with d2 > D^2 is no neighbour.  A target with fewer than k neighbours (also k > n_src) has
    index -1 and weight 0 in the unused slots; a target with none is invalid and receives ``fill_value``.

    Agreement with the reference's ``resample_to_grid`` is not pinned: VTK's probe filter interpolates inside the containing
    cell on the mesh's connectivity, which this package never has.  What is pinned is 'nearest' against scipy.

    Attributes: ``index`` (n_dst, k) int64, ``weight`` and ``d2`` (n_dst, k) float64, ``valid`` (n_dst,) bool -- device tensors;
    ``n_src``, ``n_dst``, ``method``, ``k``; ``info_``: bin counts, largest bin occupancy, number of invalid targets, mean and
    maximum number of candidate points inspected per target.  Pickles as host arrays and is uploaded again at its next use."""

    METHODS = ('nearest', 'idw')

    def __init__(self, xyz_src, dst, method='nearest', k=8, max_distance=None, engine=None, power=2):
        _refuse_sharded(xyz_src, dst)
        if method not in self.METHODS:
            raise ValueError(f'method must be one of {self.METHODS}, got {method!r}')
        if power != 2:
            raise ValueError(f'power {power!r}: inverse-distance weights are built for power 2 only')
        if isinstance(k, bool) or k != int(k) or not 1 <= int(k) <= 8:
            raise ValueError(f'k must be an integer in 1 .. 8, got {k!r}')
        if max_distance is not None and not float(max_distance) >= 0:
            raise ValueError(f'max_distance must be a distance >= 0 or None, got {max_distance!r}')
        src = _cloud(xyz_src, 'xyz_src')
        if isinstance(dst, RectilinearGrid):                      # its centres as a point cloud, see the class docstring
            dst = dst.cell_centers()
        target = dst if isinstance(dst, VoxelGrid) else _cloud(dst, 'dst')
        self.method = method
        self.k = 1 if method == 'nearest' else int(k)
        self.max_distance = None if max_distance is None else float(max_distance)
        self.n_src = int(src.shape[0])
        self.n_dst = int(target.n_cells if isinstance(dst, VoxelGrid) else target.shape[0])
        if engine is None:
            from .engine import HipEngine
            engine = HipEngine()
        self._eng = engine
        plan = engine.resample_plan(src, target, self.k, method, self.max_distance)
        self.index, self.weight, self.d2 = plan['index'], plan['weight'], plan['d2']
        seen = np.asarray(engine.to_host(plan['inspected']))
        first = np.asarray(engine.to_host(self.index[:, 0].contiguous()))
        self.info_ = dict(bins=tuple(int(b) for b in plan['bins']), max_bin_occupancy=int(plan['max_bin']),
                          n_invalid=int(np.count_nonzero(first < 0)), inspected_mean=float(seen.mean()),
                          inspected_max=int(seen.max()))

    # ------------------------------------------------------------------ storage
    @classmethod
    def _from_host(cls, index, weight, d2, n_src, method, k, max_distance, info):
        self = cls.__new__(cls)
        self.index, self.weight, self.d2 = index, weight, d2
        self.n_src, self.n_dst, self.method, self.k, self.max_distance = int(n_src), int(index.shape[0]), method, int(k), max_distance
        self.info_, self._eng = dict(info), None
        return self

    def _engine(self, engine=None):
        if engine is not None and self._eng is None:
            self._eng = engine
        if self._eng is None:
            from .engine import HipEngine
            self._eng = HipEngine()
        return self._eng

    def tensors(self, engine=None):
        """(index, weight, d2) as tensors of the engine; host arrays (after unpickling) are uploaded once"""
        if isinstance(self.index, np.ndarray):
            eng = self._engine(engine)
            self.index = eng.to_device(self.index, dtype=eng.torch.int64)
            self.weight, self.d2 = eng.to_device(self.weight), eng.to_device(self.d2)
        return self.index, self.weight, self.d2

    @property
    def valid(self):
        """(n_dst,) bool: the target has at least one neighbour"""
        return self.index[:, 0] >= 0

    def __reduce__(self):
        if isinstance(self.index, np.ndarray):
            host = (self.index, self.weight, self.d2)
        else:
            eng = self._engine()
            host = tuple(np.array(eng.to_host(t)) for t in (self.index, self.weight, self.d2))
        return (Resampler._from_host, (*host, self.n_src, self.method, self.k, self.max_distance, self.info_))

    # ------------------------------------------------------------------ application
    def apply(self, X, n_features, *, fill_value=0.0, out=None, to_host=None, engine=None):
        """``X_int[f * n_dst + c, :] = sum_j weight[c, j] * X[f * n_src + index[c, j], :]`` for the ``n_features`` blocks of the
        feature-major snapshot matrix ``X`` (n_features * n_src, m), summed for j = 0, 1, ... in float64; float32 storage is
        widened on load and rounded once on store, the result has the dtype of ``X``.  'nearest' copies the row: NaN, -0.0 and
        every other bit pattern arrive unchanged.  An invalid target gets ``fill_value`` in every feature and column.

        ``X``: an ndarray (float64 or float32, uploaded as stored), a device tensor or a ``DeviceMatrix``.  ndarray in,
        ndarray out; a ``DeviceMatrix`` in gives a ``DeviceMatrix`` that ``SPR(...)`` takes as it is; a tensor gives a tensor.
        ``to_host`` overrides (True: an ndarray; False: what stays in HBM).  ``out``: a device view of shape
        (n_features * n_dst, m) and the dtype of ``X``, contiguous columns and any row stride -- a column block of a wider
        matrix, which is what a loop over simulations on different meshes writes into."""
        from .rom import DeviceMatrix
        _refuse_sharded(X, out)
        n_features = int(n_features)
        if n_features < 1:
            raise ValueError('n_features must be at least 1')
        eng = self._engine(engine)
        t = eng.torch
        index, weight, _ = self.tensors(eng)
        kind = 'matrix' if isinstance(X, DeviceMatrix) else 'tensor' if isinstance(X, t.Tensor) else 'host'
        if kind == 'host':
            X = np.asarray(X)
            if X.dtype not in (np.float64, np.float32):
                X = X.astype(np.float64)
        xt = X.tensor if kind == 'matrix' else X
        vector = xt.ndim == 1
        if vector:
            xt = xt.reshape(-1, 1)
        if xt.ndim != 2 or xt.shape[0] != n_features * self.n_src:
            raise ValueError(f'X must have n_features * n_src = {n_features} * {self.n_src} rows, got shape {tuple(xt.shape)}')
        if kind == 'host':
            xt = eng.to_device(xt, dtype=t.float32 if xt.dtype == np.float32 else t.float64)
        res = eng.resample_apply(xt, self.n_src, n_features, index, weight, self.method, fill_value, out)
        if vector and out is None:
            res = res.reshape(-1)
        if to_host is None:
            to_host = kind == 'host' and out is None
        if to_host:
            return np.array(eng.to_host(res.contiguous()))
        if kind == 'tensor' or out is not None:
            return res
        return DeviceMatrix(res, basis=X.basis if kind == 'matrix' else None)

    def operator(self, feature=0, n_features=1, to_host=True):
        """The operator as a matrix of shape (n_dst, n_features * n_src), its columns in the block of ``feature``: a
        ``scipy.sparse.csr_matrix``, or with ``to_host=False`` a ``DeviceCSR``.  Column indices ascend in every row; the row
        of an invalid target is empty.  For checks, and for users who want the matrix."""
        n_features, f = int(n_features), int(feature)
        if n_features < 1 or not 0 <= f < n_features:
            raise ValueError(f'feature {feature} is outside the {n_features} feature blocks')
        eng = self._engine()
        t = eng.torch
        index, weight, _ = self.tensors(eng)
        used = index >= 0
        cols, order = t.sort(t.where(used, index, t.full_like(index, 2 ** 62)), dim=1, stable=True)
        vals = t.gather(weight, 1, order)
        used = cols < 2 ** 62
        indptr = t.zeros((self.n_dst + 1,), dtype=t.int64, device=index.device)
        t.cumsum(used.sum(dim=1), 0, out=indptr[1:])
        C = DeviceCSR(indptr, cols[used] + f * self.n_src, vals[used], (self.n_dst, n_features * self.n_src), engine=eng)
        return C.tocsr() if to_host else C


def resample_to_grid(mesh, X, dimensions, verbose=False, *, method='nearest', k=8, max_distance=None, fill_value=0.0,
                     to_host=None, engine=None):
    """Reference :17-99 samples the fields of a pyvista mesh on a structured grid.  Here ``mesh`` is the (n_cells, 3) array of
    the cell centres of the source mesh, ``X`` the (n_features * n_cells, m) snapshot matrix (ndarray, device tensor or
    ``DeviceMatrix``; ``n_features = X.shape[0] // n_cells`` as in the reference, a remainder is a ``ValueError``) and
    ``dimensions`` a ``VoxelGrid``, a ``RectilinearGrid`` (stretched axes: the only way into the rectilinear path), or the
    three coordinate arrays of the reference's second form, read by ``VoxelGrid.from_axes`` (uniform steps, a ``ValueError``
    otherwise).  Returns ``(grid, X_int, xyz_int)``: the reference's triple with the grid object -- the one passed in, if one
    was -- in place of the pyvista mesh, ``X_int`` (n_features * n_grid_cells, m) of the kind ``Resampler.apply`` returns for
    ``X``, ``xyz_int`` the grid's cell centres.  ``method``, ``k``, ``max_distance``, ``fill_value``: see ``Resampler``.

    The numbers are NOT those of the reference: VTK's probe filter interpolates inside the containing cell, which needs the
    connectivity of the mesh; this is nearest-neighbour or inverse-distance resampling of the cell centres.  Anything but an
    (n_cells, 3) array as ``mesh`` (a pyvista object, None) raises ``NotImplementedError``, and so does the reference's first
    form of ``dimensions``, three cell counts: it spans the bounds of the MESH, which cell centres do not give -- describe
    the grid with ``VoxelGrid(origin, spacing, dims)``."""
    if not (isinstance(mesh, (np.ndarray, list, tuple)) and np.ndim(mesh) == 2 and np.shape(mesh)[1] == 3):
        raise NotImplementedError('resample_to_grid takes the (n_cells, 3) cell centres of the source mesh; pyvista meshes '
                                  '(reference utils.py:17-99) are outside this implementation.')
    if isinstance(dimensions, (VoxelGrid, RectilinearGrid)):
        grid = dimensions
    elif isinstance(dimensions, (list, tuple, np.ndarray)) and len(dimensions) == 3 and all(np.ndim(d) == 0 for d in dimensions):
        raise NotImplementedError('three cell counts span the bounds of the mesh (reference utils.py:17-99), which cell '
                                  'centres do not give: describe the grid with VoxelGrid(origin, spacing, dims).')
    elif isinstance(dimensions, (list, tuple)) and len(dimensions) == 3:
        grid = VoxelGrid.from_axes(*dimensions)
    else:
        raise ValueError('dimensions must be a VoxelGrid, a RectilinearGrid or three coordinate arrays')
    _refuse_sharded(X)
    n_cells = int(np.shape(mesh)[0])
    rows = int(X.shape[0]) if hasattr(X, 'shape') else int(np.shape(X)[0])
    if n_cells == 0 or rows % n_cells or rows == 0:
        raise ValueError(f'X has {rows} rows, which is no multiple of the {n_cells} cells of the mesh')
    n_features = rows // n_cells
    rs = Resampler(mesh, grid, method=method, k=k, max_distance=max_distance, engine=engine)
    if verbose:
        print(f'Resampling {n_features} features of {n_cells} cells onto {grid.n_cells} cells ({method}): {rs.info_}', flush=True)
    X_int = rs.apply(X, n_features, fill_value=fill_value, to_host=to_host)
    return grid, X_int, grid.cell_centers()
