"""DeviceCSR: a sparse measurement matrix whose three CSR arrays live in HBM."""
from __future__ import annotations

import numpy as np

__all__ = ['DeviceCSR']


class DeviceCSR:
    """An (s, n) CSR matrix held as device tensors ``indptr`` (s + 1,), ``indices`` (nnz,), both int64, and ``vals``
    (nnz,) float64, column indices ascending in every row (the form ``ROM._csr_device`` gives a scipy.sparse matrix with
    ``sort_indices()``).  ``camera.project(to_host=False)`` returns one, and ``train(C)``, ``reconstruct(sampling=C)`` and
    ``unscale_data(sampling=C)`` take it as it is: the chain camera -> C -> train -> predict -> reconstruct never leaves HBM.

    Column indices are GLOBAL rows of the snapshot matrix.  A row-sharded object takes the same DeviceCSR on every rank
    (every rank casts the same rays): the measure kernel skips the columns outside the rank's rows and the partial
    products are all-reduced like those of any other C, so building the matrix needs no collective.

    It pickles as its host arrays and is uploaded again when it is first used."""

    def __init__(self, indptr, indices, vals, shape, engine=None):
        self.indptr, self.indices, self.vals = indptr, indices, vals
        self.shape = (int(shape[0]), int(shape[1]))
        self._eng = engine
        if self.indptr.shape[0] != self.shape[0] + 1 or self.indices.shape[0] != self.vals.shape[0]:
            raise ValueError('indptr must have one entry more than rows, indices and vals one per stored element')

    ndim = 2

    @property
    def nnz(self):
        return int(self.indices.shape[0])

    def _engine(self, engine=None):
        if engine is not None and self._eng is None:
            self._eng = engine
        if self._eng is None:
            from .engine import HipEngine
            self._eng = HipEngine()
        return self._eng

    def tensors(self, engine=None):
        """(indptr, indices, vals) as tensors of the engine; host arrays (after unpickling) are uploaded once"""
        if isinstance(self.indptr, np.ndarray):
            eng = self._engine(engine)
            t = eng.torch
            self.indptr, self.indices = eng.to_device(self.indptr, dtype=t.int64), eng.to_device(self.indices, dtype=t.int64)
            self.vals = eng.to_device(self.vals)
        return self.indptr, self.indices, self.vals

    def _host(self):
        if isinstance(self.indptr, np.ndarray):
            return self.indptr, self.indices, self.vals
        eng = self._engine()
        return tuple(np.array(eng.to_host(t)) for t in (self.indptr, self.indices, self.vals))

    def tocsr(self):
        """the same matrix as a scipy.sparse.csr_matrix on the host"""
        import scipy.sparse as sp
        indptr, indices, vals = self._host()
        return sp.csr_matrix((vals, indices, indptr), shape=self.shape)

    def dot(self, x):
        """C . x for an (n,) host vector -> (s,) host vector, on the device: the measure kernel without a basis
        (spr_measure_csr_f64, r = 0), whose second output is C . v for any vector v."""
        x = np.asarray(x, dtype=np.float64)
        if x.shape != (self.shape[1],):
            raise ValueError(f'shapes {self.shape} and {x.shape} not aligned')
        eng = self._engine()
        indptr, indices, vals = self.tensors()
        _, y = eng.measure_csr(indptr, indices, vals, None, 0, eng.to_device(x))
        return np.array(eng.to_host(y))

    @classmethod
    def vstack(cls, blocks):
        """the rows of several matrices with the same column count, one after the other (several cameras)"""
        blocks = list(blocks)
        if not blocks or any(not isinstance(b, DeviceCSR) for b in blocks):
            raise ValueError('vstack takes a non-empty list of DeviceCSR')
        if any(b.shape[1] != blocks[0].shape[1] for b in blocks):
            raise ValueError('vstack: the blocks differ in their column count')
        eng = blocks[0]._engine()
        t = eng.torch
        parts, base = [], 0
        for k, b in enumerate(blocks):
            indptr = b.tensors(eng)[0]
            parts.append((indptr if k == 0 else indptr[1:]) + base)
            base += b.nnz
        return cls(t.cat(parts), t.cat([b.indices for b in blocks]), t.cat([b.vals for b in blocks]),
                   (sum(b.shape[0] for b in blocks), blocks[0].shape[1]), engine=eng)

    def __reduce__(self):
        return (DeviceCSR, (*self._host(), self.shape))
