"""The class surface: ROM and SPR with the constructor, methods, defaults, return shapes and exception types of
``openmeasure.sparse_sensing`` (reference: src/openmeasure/sparse_sensing.py) over the engine -- see sparse_sensing.py for the
map of reference call sites to kernels.  Host eigen routes: _eigen.py; placement drivers and GEM: _placement.py; sharding,
collectives and the field exchange: _shard.py."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import _eigen
from ._csr import DeviceCSR
from ._design import DesignPlacement
from ._lib import SPR_MAX_R, SPR_MAX_R_WIDE
from ._placement import GemPlacement, _check_mask, pivot_loop
from ._shard import PendingField, RowShard, ShardedOps

__all__ = ['ROM', 'SPR', 'RowShard', 'DeviceMatrix', 'PendingField', 'OneHotRows']

_DEVICE_SPECTRUM_MAX_M = 24   # above this the single-workgroup Jacobi is slower than host dsyevd (csrc/spectrum.hip)
# Gram route (fit): singular vectors come from the eigenvectors of X0^T X0, whose rounding error eps * sigma_1^2 reaches
# mode i as eps * (sigma_1/sigma_i)^2.  Up to this ratio the basis is as good as LAPACK's to ~1e-8 (sensor parity
# verified on reference fixtures); above it fit() runs the refinement pass of _refine_spectrum (one more read of X).
_GRAM_KAPPA_REFINE = 1e4
_GRAM_REFINE_MAX_PASSES = 3
_DENSE_C_LIMIT = 1 << 26   # optimal_placement returns a dense ndarray below this many bytes (64 MiB)


class DeviceMatrix:
    """A snapshot block that already lives in HBM (2-D float64 or float32 CUDA tensor, rows contiguous).
    float32 = storage precision only: every kernel widens on load and computes in f64, and the basis Ur is float64
    like the reference's (its X0 = (X - X_cnt)/X_scl is float64 for any dtype of X because X_cnt / X_scl are, :106-107,
    :169, and np.linalg.svd :272 keeps that dtype).  ``basis='f32'`` stores the basis in float32 as well -- a storage
    option the reference does not have, for shards whose f64 basis would not fit (BASELINE config 5: 204.8 GB shard +
    51.2 GB f32 basis per GPU); the sensors are then those of the stored basis and ``pivot_gap_`` says how far each
    pick was from a tie."""

    def __init__(self, tensor, basis=None):
        if basis not in (None, 'f64', 'f32'):
            raise ValueError("basis must be None / 'f64' / 'f32'")
        self.tensor = tensor
        self.basis = 'f32' if basis == 'f32' else 'f64'
        if self.basis == 'f32' and str(tensor.dtype) != 'torch.float32':
            raise ValueError("basis='f32' is a storage option of a float32 snapshot block")

    @property
    def shape(self):
        return tuple(self.tensor.shape)


class OneHotRows:
    """The one-hot measurement matrix C of ``optimal_placement`` (reference :741-743: ``C = np.zeros((s, n));
    C[j, P[j]] = 1``) held as its s row indices instead of s x n doubles -- 46 GB at BASELINE config 3, 819 GB at
    config 5.  ``optimal_placement`` returns the plain ndarray while it is small (64 MiB) and this object above that;
    it behaves like the dense matrix for everything the reference's documentation does with C (README.md:165-184):

        np.argmax(C[i, :])          C @ x, C.dot(x)  (x of shape (n,) or (n, k))        C.shape, len(C)
        np.argmax(C, axis=1)        spr.train(C)                                         np.asarray(C), C.toarray()

    ``np.asarray`` / ``toarray`` build the dense matrix only below ``dense_limit`` bytes (MemoryError beyond: that
    allocation is what this class exists to avoid); ``tocsr()`` gives a scipy.sparse matrix of any size.  ``rows`` are
    the ordered global sensor rows (= ``spr.sensors_``).  A 1-D instance (shape (n,)) is what ``C[i, :]`` returns."""

    dense_limit = 1 << 32
    dtype = np.dtype(np.float64)
    __array_priority__ = 20.0                                  # ndarray @ OneHotRows defers to __rmatmul__

    def __init__(self, rows, n, _vector=False):
        self.rows = np.asarray(rows, dtype=np.int64).reshape(-1)
        self.n = int(n)
        self._vector = bool(_vector)
        if self._vector and self.rows.size != 1:
            raise ValueError('a one-hot vector has exactly one non-zero')
        if self.rows.size and (self.rows.min() < 0 or self.rows.max() >= self.n):
            raise IndexError('sensor row outside [0, n)')

    @property
    def shape(self):
        return (self.n,) if self._vector else (self.rows.size, self.n)

    @property
    def ndim(self):
        return 1 if self._vector else 2

    @property
    def nnz(self):
        return int(self.rows.size)

    def __len__(self):
        return self.shape[0]

    def __repr__(self):
        return f'OneHotRows(shape={self.shape}, rows={self.rows.tolist() if self.rows.size <= 16 else "..."})'

    # ---- what NumPy asks for -------------------------------------------------------------------------------
    def argmax(self, axis=None, out=None, **kw):
        """np.argmax(C[i, :]) -> the sensor's row; np.argmax(C, axis=1) -> all of them (1-D); axis=None: flat index."""
        if self._vector:
            if axis not in (None, 0, -1):
                raise np.exceptions.AxisError(axis, 1)
            return np.int64(self.rows[0])
        if axis in (1, -1):
            return self.rows.copy()
        if axis is None:                                       # first maximum of the flattened matrix: row 0's one
            return np.int64(self.rows[0]) if self.rows.size else np.int64(0)
        if axis in (0, -2):
            raise MemoryError('argmax over axis 0 of the one-hot matrix needs its n columns; use tocsr()')
        raise np.exceptions.AxisError(axis, 2)

    def __array__(self, dtype=None, copy=None):
        nbytes = 8 * self.n * (1 if self._vector else self.rows.size)
        if nbytes > self.dense_limit:
            raise MemoryError(f'dense form of this one-hot matrix needs {nbytes / 2 ** 30:.1f} GiB; use its row indices '
                              '(.rows / np.argmax(C, axis=1)), C @ x, or C.tocsr()')
        if self._vector:
            out = np.zeros(self.n)
            out[self.rows[0]] = 1.0
        else:
            out = np.zeros((self.rows.size, self.n))
            out[np.arange(self.rows.size), self.rows] = 1.0
        return out if dtype is None else out.astype(dtype, copy=False)

    def toarray(self):
        return self.__array__()

    def tocsr(self):
        import scipy.sparse as sp
        s = self.rows.size
        return sp.csr_matrix((np.ones(s), self.rows, np.arange(s + 1)), shape=(s, self.n))

    def sum(self, axis=None):
        if self._vector or axis is None:
            return np.float64(self.rows.size)
        if axis in (1, -1):
            return np.ones(self.rows.size)
        return np.bincount(self.rows, minlength=self.n).astype(np.float64)   # axis 0: (n,), allocated by request

    # ---- indexing: C[i, :], C[i], C[i, j], C[a:b] ----------------------------------------------------------
    def __getitem__(self, key):
        if self._vector:
            if isinstance(key, (int, np.integer)):
                k = int(key) + (self.n if key < 0 else 0)
                if not 0 <= k < self.n:
                    raise IndexError('index out of range')
                return np.float64(1.0 if k == self.rows[0] else 0.0)
            return np.asarray(self)[key]
        if isinstance(key, tuple):
            if len(key) != 2:
                raise IndexError('too many indices for a 2-D matrix')
            ri, ci = key
        else:
            ri, ci = key, slice(None)
        full_cols = isinstance(ci, slice) and ci == slice(None)
        if isinstance(ri, (int, np.integer)):
            row = self.rows[ri]                                # IndexError like ndarray when out of range
            if full_cols:
                return OneHotRows([row], self.n, _vector=True)
            if isinstance(ci, (int, np.integer)):
                k = int(ci) + (self.n if ci < 0 else 0)
                if not 0 <= k < self.n:                        # the dense matrix this stands in for raises as well
                    raise IndexError(f'index {int(ci)} is out of bounds for axis 1 with size {self.n}')
                return np.float64(1.0 if k == row else 0.0)
            return np.asarray(OneHotRows([row], self.n, _vector=True))[ci]
        if full_cols:
            return OneHotRows(self.rows[ri], self.n)           # row slice / index array: still one-hot rows
        return np.asarray(self)[key]                            # column subsets: dense (size-guarded)

    # ---- products ------------------------------------------------------------------------------------------
    def dot(self, x):
        """C.dot(x) = the sampled entries x[rows] (reference :797, :573 and README.md:176)."""
        x = np.asarray(x)
        if x.ndim == 0 or x.shape[0] != self.n:
            raise ValueError(f'shapes {self.shape} and {x.shape} not aligned')
        return x[self.rows[0]] if self._vector else x[self.rows]

    __matmul__ = dot

    def __rmatmul__(self, a):
        return np.asarray(a) @ np.asarray(self)                 # (k, s) @ (s, n): dense by nature, size-guarded

    @property
    def T(self):
        return self.tocsr().T


#: what a fitted object holds of its row block, in the order the engine methods that work on the basis take it first:
#: eng.reconstruct(*blk, A_d), eng.encode(*blk, Xd), ...  (ROM._block builds it)
FittedBlock = namedtuple('FittedBlock', 'Ur row0 n_points n_features rowmean scale')


class _Trace:
    """Optional per-phase wall-clock trace of fit() (SPR_TRACE=1): synchronises at every mark."""

    def __init__(self, eng):
        import os
        self.on = os.environ.get('SPR_TRACE', '0') == '1'
        self.eng = eng
        self.marks = []
        if self.on:
            self.mark('start')

    def mark(self, label):
        if not self.on:
            return
        import time
        if hasattr(self.eng, 'device') and self.eng.device.type == 'cuda':
            self.eng.torch.cuda.synchronize()
        self.marks.append((label, time.perf_counter()))

    def report(self):
        if not self.on:
            return
        import sys
        t0 = self.marks[0][1]
        prev = t0
        parts = []
        for label, t in self.marks[1:]:
            parts.append(f'{label}={1e3 * (t - prev):.2f}')
            prev = t
        print('[spr trace] ' + ' '.join(parts) + f' total={1e3 * (prev - t0):.2f} ms', file=sys.stderr)


class _DeviceState(dict):
    """The tensors an object keeps in HBM, by name.  An unpickled object starts with host copies only (``stash``): an
    entry is uploaded when it is first asked for, so loading a pickle needs no GPU until the object is used."""

    def __init__(self, stash=None, upload=None):
        super().__init__()
        self.stash = dict(stash or {})
        self.upload = upload
        #: ROM.defer_project: the entries a launch that fit() only RECORDED will write ('Ur', 'nrm0'), and the function that
        #: enqueues it.  Every read of such an entry -- whoever makes it, through whichever method -- runs ``guard`` first.
        self.promised = ()
        self.guard = None

    def _keep_promise(self, key=None):
        if self.promised and (key is None or key in self.promised):
            self.guard()                                      # (clears ``promised``)

    def __getitem__(self, key):
        self._keep_promise(key)
        return dict.__getitem__(self, key)                    # (-> __missing__ for a stashed entry)

    def __missing__(self, key):
        if key in self.stash:
            t = self[key] = self.upload(self.stash.pop(key))
            return t
        raise KeyError(key)

    def __contains__(self, key):
        return dict.__contains__(self, key) or key in self.stash or key in self.promised

    def get(self, key, default=None):
        try:
            return self[key]
        except KeyError:
            return default

    def items(self):
        self._keep_promise()
        return dict.items(self)

    def values(self):
        self._keep_promise()
        return dict.values(self)

    def pop(self, key, *default):
        self._keep_promise(key)
        if not dict.__contains__(self, key) and key in self.stash:
            # every pop in this module either discards the entry or wants a BUFFER to overwrite: a host copy is neither
            del self.stash[key]
            if default:
                return default[0]
            raise KeyError(key)
        return dict.pop(self, key, *default)


#: attributes that never travel in a pickle: the engine, device state (downloaded instead), events, in-flight work
_TRANSIENT = ('_eng', '_d', '_trace', '_pending', '_pending_field', '_gram_events', '_gram_events_pending', '_layout_src',
              '_gap_t0', '_G', '_last_decomp', 'comm_timing', 'last_comm_', '_layout', '_p2p', '_gather_sel', '_basis_checked', '_basis_diverged', '_deferred', '_proj_pending', '_ur_spare', '_row0_d', '_ncomm', '_combined', '_comm_stream')


class ROM(ShardedOps):
    """Reduced-order-model utilities (reference: ROM, sparse_sensing.py:18-511)."""

    def __init__(self, X, n_features, xyz, shard=None, engine=None):
        # reference :69-81 -- same checks, same exception types, in the same order
        if isinstance(X, DeviceMatrix):
            pass
        elif type(X) is not np.ndarray:
            raise TypeError('The matrix X is not a numpy array.')
        if type(n_features) is not int:
            raise TypeError('The parameter n_features is not an integer.')
        self.X = X
        self.n_features = n_features
        self.xyz = xyz
        self._shard = shard
        n = shard.n_global if shard is not None else X.shape[0]
        self.n_points = n // self.n_features
        if n % self.n_features != 0:
            raise Exception('The number of rows of X is not a multiple of n_features')
        self._n_global = n
        self._row0 = shard.row0 if shard is not None else 0
        if self._row0 + X.shape[0] > n:
            raise ValueError('The local row block does not fit in the global matrix.')
        self._eng = engine
        self._d = _DeviceState()    # device-resident state
        self._host = {}         # lazily downloaded copies

    # ------------------------------------------------------------------ reference methods outside the built path
    #: CPOD (_cpod.py): a row counts as violated when it exceeds its scaled limit by more than cpod_tol (scaled units, i.e.
    #: multiples of X_scl); at most cpod_rows_per_round (<= 256) rows join a snapshot's working set per sweep; CPOD raises
    #: RuntimeError rather than return an unconverged snapshot after cpod_max_rounds sweeps or beyond cpod_max_rows working
    #: rows.  Meaning and defaults of SPR's cols_* knobs.
    cpod_tol = 1e-9
    cpod_rows_per_round = 64
    cpod_max_rounds = 60
    cpod_max_rows = 4000

    def CPOD(self, problem_dict, **kwargs):
        """Reference :434-461: the constrained POD solves one cvxpy problem per snapshot and puts the solutions into Ar / Vr.
        Built for the problem its documentation states (docs/gpr_doc.ipynb): ``problem_dict = {'limits': [lo, hi]}`` with
        per-feature limits in raw units, as scale_limits takes them --

            minimise || Ur g - X0[:, i] ||_2   subject to   lo0 <= Ur g <= hi0        for every snapshot i

        by constraint generation on the device (_cpod.py); diagnostics in ``cpod_info_``, an infeasible snapshot is a row
        of NaN.  Keyword arguments name cvxpy back ends (solver=, verbose=, max_iter= ...): stored, not used.  A dict of
        cvxpy objects ('problem' / 'g' / 'x0', the reference's own form) has no device path: raises, like every option
        without one.

        Two limits of the identity |Ur g - X0[:, i]|^2 = |g - Ar[i]|^2 + const the path rests on:
        * the mark fit() leaves says WHO computed the basis, not how orthonormal it is.  fit() takes Ur from the
          eigenvectors of the Gram matrix, so Ur^T Ur - I grows as eps (sigma_1 / sigma_r)^2: for a truncation that keeps
          modes down to sigma_r ~ 1e-6 sigma_1 the objective minimised here differs from the reference's at the 1e-4
          level, the way it does for the refused f32-stored basis.  Nothing checks this; keep sigma_r / sigma_1 well
          above sqrt(eps) ~ 1e-8, or verify Ur^T Ur yourself.
        * the centre is the Ar of the fit, copied to ``_cpod_Ar0`` at the first call and kept until the next fit().  An
          assignment to ``rom.Ar`` AFTER a first CPOD call is therefore ignored by later calls (before the first call it
          becomes the centre)."""
        self._flush_deferred()
        if not isinstance(problem_dict, dict) or 'limits' not in problem_dict:
            raise NotImplementedError("CPOD (constrained POD, reference :434-461) is built for problem_dict = {'limits': [lo, "
                                      "hi]} (per-feature limits on the reconstruction); a dict of cvxpy objects ('problem', "
                                      "'g', 'x0') is not part of this implementation.")
        eng = self._engine()
        if not hasattr(eng, 'bound_sweep'):
            raise NotImplementedError("CPOD needs the engine's bound sweep (csrc/bounds.hip); this engine has none (no CPU "
                                      'fallback).')
        self._fitted('Ur', 'Ur')
        why = self.__dict__.get('_basis_foreign', 'no fit() of this object computed the basis')
        if why is not None:
            raise NotImplementedError('CPOD minimises |g - Ar[i]|^2, which equals the reference\'s |Ur g - X0[:, i]|^2 only for '
                                      f'the orthonormal basis fit() computed together with Ar: {why}.')
        self.cpod_kwargs = dict(kwargs)
        Ar0 = self.__dict__.get('_cpod_Ar0')
        if Ar0 is None:
            Ar0 = self._cpod_Ar0 = np.array(self.Ar, dtype=np.float64)      # (m <= 24 device fit: materialises)
        from ._cpod import constrain_pod
        Gr = constrain_pod(self, problem_dict['limits'], Ar0)
        self.Ar = Gr
        self.Vr = Gr / self.Sigma_r                                         # :456-461, Sigma_r unchanged

    def _feature_cnt_minmax(self):
        """(F, 2) per-feature min / max of X_cnt over ALL ranks' rows: decides the +-1000 clamps of scale_limits (:201-204)
        for the whole feature block"""
        eng = self._engine()
        mean_d = self._fitted('rowmean', 'X_cnt')
        mm = self._all_gather(eng.feature_minmax(mean_d.view(-1, 1), self._row0, self.n_points, self.n_features))
        mm = eng.to_host(mm)                              # (world, F, 2)
        return np.stack([mm[:, :, 0].min(axis=0), mm[:, :, 1].max(axis=0)], axis=1)

    def adaptive_sampling(self, P, scale_type='std'):
        """Reference :377-432.  Not built: its snapshot weights contain Vt[k,:] @ V[k,:] (:401), which changes with the
        arbitrary signs LAPACK gives the singular vectors, and its candidate points come from an unseeded Latin hypercube --
        there is no result to reproduce."""
        raise NotImplementedError('adaptive_sampling (reference :377-432) is not part of this implementation: its result '
                                  'depends on the sign convention of the singular vectors and on an unseeded sampler.')

    # ------------------------------------------------------------------ pickling (the reference's objects are plain attributes)
    def __getstate__(self):
        """What the reference's object would pickle -- X, the fitted arrays, the trained operator -- with everything that
        lives in HBM downloaded first (a DeviceMatrix becomes the host ndarray of its values; the basis comes down whole: a
        pickle of a fitted config-3 object is 230 GB, as the reference's would be).  The engine, events and in-flight
        work stay behind; a process group cannot travel either (the shard keeps its row block, group = default)."""
        self._flush_deferred()
        self._materialize()
        pf = self.__dict__.get('_pending_field')
        if pf is not None and pf.pending:
            pf.wait()
        eng = self._eng
        state = {k: v for k, v in self.__dict__.items() if k not in _TRANSIENT and not hasattr(v, 'is_cuda')}
        d_host = dict(self._d.stash)
        for k, t in self._d.items():
            if k == 'X' and not isinstance(self.X, DeviceMatrix):
                continue                                       # the host ndarray X is in the state already
            d_host[k] = eng.to_host(t)
        if isinstance(self.X, DeviceMatrix):
            state['X'] = d_host.pop('X') if 'X' in d_host else eng.to_host(self.X.tensor)
            state['_basis_f32'] = self.X.basis == 'f32'
        state['_d_host'] = d_host
        if self._shard is not None:
            sh = RowShard(self._shard.row0, self._shard.n_global, None, self._shard.force_collectives,
                          self._shard.broadcast_basis, self._shard.partial, self._shard.gather, self._shard.native_comm)
            state['_shard'] = sh
        return state

    def __setstate__(self, state):
        d_host = state.pop('_d_host', {})
        self.__dict__.update(state)
        self._eng = None                                       # the default engine, created on first use (or assign ._eng)

        def upload(a):
            eng = self._engine()
            return eng.to_device(a, dtype=eng.torch.float32 if a.dtype == np.float32 else None)
        self._d = _DeviceState(d_host, upload)

    # ------------------------------------------------------------------ lazily fetched fit results
    _LAZY = ('Ar', 'Sigma_r', 'Vr', 'exp_variance_', 'S_', '_scl_f', '_var_f')

    #: Squared row norms of the basis as a by-product of fit(): the projection that stores Ur also leaves |Ur[i, :]|^2 of
    #: every row it wrote (8 bytes per row), and optimal_placement('qr') starts from that vector instead of reading the
    #: whole basis once more (one sweep of 46 GB less at BASELINE config 3; same sensors).  None ("auto", the default of
    #: SPR): whenever the projection kernel the shape takes anyway produces them at no measurable cost (the W-stationary
    #: and the streamed-W kernel: every BASELINE shape but config 1); True: always (m <= 256 shapes outside the
    #: W-stationary kernel's range then run the streamed-W kernel); False (ROM, whose users never place sensors): never.
    placement_norms = False

    #: Gap filler (OPT-IN: ``rom.gap_filler = True`` or SPR_GAP_FILLER=1).  Between the Gram pass and the projection the
    #: device waits for the host (download of the m x m Gram matrix, eigen-solve, upload of W: 1.8 ms at m = 256, 8 ms at
    #: m = 512), and a chip that idles for a few milliseconds lowers its clock and takes several more to raise it again: the
    #: kernels of a fit() + reconstruct() step on one rank's block of BASELINE config 4 at N = 8 take 19.9 ms behind a 3 ms gap
    #: against 18.6 ms back to back (tools/keepalive_probe.py).  With the filler on, fit() queues the Gram kernel ONCE MORE
    #: over the first rows of X, sized to 85 % of the shortest host gap of the last fits, before it blocks on the download;
    #: the results are discarded.  It costs energy (about 2.5 J per fit) and, on a GPU shared with other work, their time --
    #: which is why a library must not do it unasked.  Only for m >= 128 and host gaps of at least _GAP_FILL_MIN_MS (shorter
    #: ones leave no clock drop worth filling).  Sharded objects size it from their own host-gap history: ranks with different
    #: histories queue fillers of different length in front of their projections (unmeasured on more than one GPU).
    gap_filler = False

    #: Deferred reconstruct (default since round 6; ``rom.defer_reconstruct = False`` or SPR_DEFER_RECONSTRUCT=0 switch it off).
    #: Between the Gram pass and the projection of fit() the device idles while the host eigen-solves (0.3 ms of a 1.5 ms step at
    #: BASELINE config 2, 1.8 ms of 22 on one rank's block of config 4 at N = 8).  ``reconstruct(a, to_host=False, wait=False)``
    #: -- the asynchronous form, which promises the field only behind ``PendingField.wait()`` -- therefore does not launch: the
    #: kernel (and, sharded, the push of the block to the peers) is enqueued in the host gap of the object's NEXT fit(), before
    #: that fit's projection overwrites the basis (the launch holds the basis, centre and scale tensors of the fit it was called
    #: after), or by ``wait()`` / any other method of the object, whichever comes first.  Same results, bit for bit
    #: (tools/step_stress.py, tools/p2p_stress.py run with it on); a loop fit -> reconstruct -> fit -> ... fills its gaps with
    #: useful work: config 2 1.49-1.52 -> 1.27-1.31 ms per step, one rank's block of config 4 22.3 -> 20.8-21.3 ms, config 3
    #: 158.1 -> 155.6 (profiles/r05_defer_reconstruct_ab.txt).  Every other form of reconstruct() -- the reference's host array,
    #: ``wait=True`` -- launches at once, as before.
    defer_reconstruct = True

    #: Deferred projection (``rom.defer_project = False`` or SPR_DEFER_PROJECT=0 switch it off).  A step fit() ->
    #: reconstruct(a) reads the whole basis back from HBM (n r B bytes: 46 of the 47.5 GB the reconstruct kernel moves at
    #: BASELINE config 3) to form one dot product per row -- of rows the projection held in its accumulators milliseconds
    #: earlier.  The coefficient vector is only known at reconstruct(), so fit() RECORDS the projection instead of
    #: enqueueing it, and the next call on the object launches it: ``reconstruct(A)`` with ``sampling=None`` and at most
    #: ``spr_project_field_max()`` vectors through spr_project_field_*, which writes the basis, the row norms AND the field
    #: in the one pass; anything else that needs the basis (``Ur``, pickling, optimal_placement, transform, train, the
    #: gappy / GPR / co-kriging / CPOD paths, any method that takes ``_block()``) launches the plain projection first.  A
    #: second fit() discards a projection nobody asked for.  Same results bit for bit: the fused kernel stores the basis the
    #: plain one stores, and its field is computed by the function the stand-alone reconstruct kernel uses for these shapes
    #: (csrc/field_dot.hpp).  Only for the single-device W-stationary case (m = 64/128/192/256, r = 16/32/48/64, at least 4096
    #: rows, no refinement pass, no pre-centring); sharded objects, fit(basis=...), the device-spectrum route (m <= 24),
    #: m > 256 and r > 64 launch at once as before.
    #: THE COST: between fit() returning and the next call on the object the projection HAS NOT STARTED -- the device is
    #: idle where it used to work under the caller's host code, the first access pays for the projection, and a snapshot
    #: matrix overwritten in place between the two calls is projected as it is THEN.
    defer_project = True

    def _defers_project(self):
        import os
        return bool(self.defer_project) and os.environ.get('SPR_DEFER_PROJECT') != '0'

    def _drop_project(self):
        """Forget a recorded projection (fit(): the basis it would write is about to be replaced)"""
        rec = self.__dict__.pop('_proj_pending', None)
        if rec is not None:
            self._d.promised = ()
            self._ur_spare = rec['kw'].get('out')             # the buffer stays with the object for the next projection
        return rec

    def _flush_project(self, A_d=None):
        """Launch the projection fit() recorded (defer_project), if any: the plain one, or with ``A_d`` (n_p, r) the one that
        also emits the field -> (n_p, n) tensor; None when nothing was recorded or the field cannot come from it."""
        rec = self.__dict__.pop('_proj_pending', None)
        if rec is None:
            return None
        eng = self._engine()
        self._d.promised = ()
        norms = rec['kw'].get('norms')
        field = None
        if A_d is not None:
            field, Ur_d = eng.project_field(*rec['args'], scale=self._d['scale'], A=A_d, **rec['kw'])
        else:
            Ur_d = eng.project(*rec['args'], **rec['kw'])
        self._d['Ur'] = Ur_d
        if norms is not None:
            self._d['nrm0'] = norms
        return field

    def _flush_deferred(self, project=True):
        """Launch the reconstruct a previous reconstruct(wait=False) deferred (defer_reconstruct); -> True if there was one.
        ``project``: a projection fit() recorded (defer_project) is launched too, in its plain form -- every method that
        calls this touches the fitted state; reconstruct() alone passes False and decides itself."""
        if project:
            self._flush_project()
        pf = self.__dict__.pop('_deferred', None)
        if pf is not None and not pf.launched:
            pf.launch()
            return True
        return False
    _GAP_FILL_FRACTION = 0.85
    _GAP_FILL_MIN_M = 128
    #: ... and only when the host gap is long enough for the clock to matter: behind a 2.8 ms gap the filler took 0.7 ms off a
    #: 23 ms step, behind the 1.8 ms gap the batched eigen-solve leaves at m = 256 it changes nothing (same-box A/B, three
    #: repetitions: 21.98-22.37 vs 22.09-22.13 ms).  Hosts whose eigen-solve takes longer (other CPUs, loaded machines) fill, and so
    #: do wide matrices: behind the 7.6 ms eigen-solve of m = 512 the filler takes 1.6 ms off a 35 ms projection (c5s 114.0 -> 112.4 ms).
    _GAP_FILL_MIN_MS = 2.2

    #: Collective timing (bench.py): set to a dict and every collective of fit() / reconstruct() appends a pair of
    #: engine timing events (recorded on the stream the collective is ordered on) under 'allreduce' (the ONE all-reduce
    #: of fit), 'gather' (reconstruct's field all-gather when it is joined inside the call) or 'gather_exposed' (the
    #: join of a gather that was left in flight, PendingField.wait(): what of it did NOT hide under the next pass).
    comm_timing = None

    def _comm_bracket(self, key):
        """-> a function that closes the bracket opened now (no-op when comm_timing is off)."""
        ct = self.comm_timing
        eng = self._engine()
        if ct is None or not hasattr(eng, 'timing_event'):
            return lambda: None
        e0 = eng.timing_event()

        def close():
            ct.setdefault(key, []).append((e0, eng.timing_event()))
        return close

    def __getattr__(self, name):
        # only reached when normal lookup fails: results of the sync-free device fit (m <= 64) stay in HBM
        # until somebody reads them
        pend = self.__dict__.get('_pending')
        if pend is not None and name in ROM._LAZY:
            self._materialize()
            if name in self.__dict__:
                return self.__dict__[name]
        raise AttributeError(f"'{type(self).__name__}' object has no attribute '{name}'")

    def _materialize(self):
        """One D2H round trip for everything the device spectrum left in HBM."""
        pend = self.__dict__.pop('_pending', None)
        if pend is None:
            return
        eng = self._engine()
        r = pend['r']
        feat = eng.to_host(pend['feat'])
        S = eng.to_host(pend['S'])
        V = eng.to_host(pend['V'])
        self._scl_f = feat[:, 3].copy()
        self._var_f = self._scl_f ** 2
        self.S_ = S
        self.exp_variance_ = eng.to_host(pend['expvar'])[:r].copy()
        self.Ar = eng.to_host(pend['Ar'])
        self.Sigma_r = np.linalg.norm(self.Ar, axis=0)         # :504-508
        Vr = V[:, :r]
        self.Vr = Vr * (np.linalg.norm(Vr, axis=0) ** -1)

    # ------------------------------------------------------------------ plumbing
    def _engine(self):
        if self._eng is None:
            from .engine import HipEngine
            self._eng = HipEngine()
        return self._eng

    def _Xd(self):
        if 'X' not in self._d:
            eng = self._engine()
            if isinstance(self.X, DeviceMatrix):
                self._d['X'] = self.X.tensor
            else:
                if self.X.ndim < 2:
                    # the reference's first touch of X's columns is x = X[i n_points:(i+1) n_points, :] (:110): NumPy's text
                    raise IndexError(f'too many indices for array: array is {self.X.ndim}-dimensional, but 2 were indexed')
                if self.X.ndim != 2:
                    # ... and for more dimensions np.average(x, axis=1) no longer fits the n_points rows it is assigned to (:112)
                    shp = ','.join(str(d) for d in (self.n_points,) + tuple(self.X.shape[2:]))
                    raise ValueError(f'could not broadcast input array from shape ({shp}) into shape ({self.n_points},)')
                # a float32 snapshot matrix stays float32 in HBM (storage only, see DeviceMatrix)
                self._d['X'] = eng.to_device(self.X, dtype=eng.torch.float32 if self.X.dtype == np.float32 else None)
        return self._d['X']

    def _norms_buffer(self, Xd, r, precenter=False):
        """The vector the projection writes the squared row norms to (see placement_norms), or None."""
        eng = self._engine()
        want = self.placement_norms
        if want is False or r > 128 or not getattr(eng, 'supports_row_norms', False):
            return None
        if want is None and not eng.project_writes_norms(Xd, r, True, precenter):
            return None
        return eng.empty((Xd.shape[0],))

    def _basis_dtype(self):
        """storage type of Ur: float64 (the reference's, for any dtype of X) unless DeviceMatrix(basis='f32')"""
        t = self._engine().torch
        f32 = (isinstance(self.X, DeviceMatrix) and self.X.basis == 'f32') or self.__dict__.get('_basis_f32', False)
        return t.float32 if f32 else t.float64

    def _lazy(self, key, make):
        if key not in self._host:
            self._host[key] = make()
        return self._host[key]

    def _fitted(self, key, attr):
        """Device-resident state `key`; before fit()/scale_data() the reference fails with AttributeError on `attr`."""
        try:
            return self._d[key]
        except KeyError:
            raise AttributeError(f"'{type(self).__name__}' object has no attribute '{attr}'") from None

    def _engine_with(self, need, src):
        """The engine, once it is known to have the methods ``need`` (kernels of csrc/``src``)"""
        eng = self._engine()
        for name in need:
            if not hasattr(eng, name):
                raise NotImplementedError(f"this engine has no '{name}' (csrc/{src}); there is no CPU fallback.")
        return eng

    def _block(self, need=(), src=None):
        """-> FittedBlock of what this object holds NOW.  Engine capability is checked first (as _engine_with does), the
        fitted state second: before fit() the reference fails with AttributeError on Ur, before scale_data() on X_cnt."""
        self._engine_with(need, src)
        self._flush_project()                                 # (defer_project; the read of 'Ur' below would do it as well)
        return FittedBlock(self._fitted('Ur', 'Ur'), self._row0, self.n_points, self.n_features,
                           self._fitted('rowmean', 'X_cnt'), self._d['scale'])

    @staticmethod
    def _coefficients(eng, A, shape_error=None, own=False):
        """The (k, r) or (r,) operand of reconstruct / reconstruction_error / reconstruct_std(sigma=) -> (k, r) on the device:
        host input is uploaded as float64, a caller's device tensor is used in place (``own``: cloned, for a launch that
        happens later).  ``shape_error(A)``: the caller's own message for an operand it cannot take, else None.  An
        operand without rows comes back as it is, not uploaded: there is nothing to launch."""
        dev = hasattr(A, 'is_cuda')
        A = A if dev else np.asarray(A, dtype=np.float64)
        if A.ndim == 1:
            A = A[None, :]
        if shape_error is not None and (why := shape_error(A)):
            raise ValueError(why)
        if A.shape[0] == 0:
            return A
        if dev:
            return A.clone() if own else A
        return eng.to_device(A)

    def _feature_rows(self):
        """per local row: its feature id (host, int) -- only used to expand per-feature scalars"""
        n_loc = self.X.shape[0]
        return (self._row0 + np.arange(n_loc)) // self.n_points

    # ------------------------------------------------------------------ fitted attributes
    @property
    def X_cnt(self):
        """(n_local, 1) row means (reference attribute set at :166)."""
        return self._lazy('X_cnt', lambda: self._engine().to_host(self._fitted('rowmean', 'X_cnt'))[:, None])

    @property
    def X_scl(self):
        """(n_local, 1) per-feature population std, repeated per row (:167)."""
        self._fitted('scale', 'X_scl')
        return self._lazy('X_scl', lambda: self._scl_f[self._feature_rows()][:, None])

    @property
    def Ur(self):
        """(n_local, r) POD basis rows held by this rank."""
        return self._lazy('Ur', lambda: np.ascontiguousarray(self._engine().to_host(self._fitted('Ur', 'Ur'), result=True)))

    @Ur.setter
    def Ur(self, value):
        # subclasses written against the reference assign the result of decomposition() (gpr.py:386):
        # that array already has its device twin; anything else is uploaded
        self._flush_deferred()
        self._d.pop('nrm0', None)                             # row norms of the basis fit() stored, not of this one
        self._basis_foreign = 'Ur was assigned'               # (CPOD)
        last = self.__dict__.get('_last_decomp')
        if last is not None and value is last[0]:
            self._d['Ur'] = last[1]
        else:
            self._d['Ur'] = self._engine().to_device(np.asarray(value, dtype=np.float64))
        self._host['Ur'] = value

    @property
    def X0(self):
        """(n_local, m) centred/scaled matrix (:169, :492); built on first access only."""
        def make():
            eng = self._engine()
            Xd, rowmean = self._Xd(), self._fitted('rowmean', 'X0')
            n, m = Xd.shape
            block = max(1, self._X0_BLOCK_BYTES // (8 * m))
            if n <= block or not hasattr(eng, '_to_host_staged'):
                return eng.to_host(eng.scale_rows(Xd, self._row0, self.n_points, self.n_features, rowmean, self._d['inv_scale']))
            # a scaled copy of a big X does not fit next to it in HBM (184 + 184 GB at BASELINE config 3): row blocks, each
            # scaled into a scratch block and streamed to its place in the host array
            out = np.empty((n, m), dtype=np.float64)
            for i0 in range(0, n, block):
                i1 = min(n, i0 + block)
                t = eng.scale_rows(Xd[i0:i1], self._row0 + i0, self.n_points, self.n_features, rowmean[i0:i1],
                                   self._d['inv_scale'])
                eng._to_host_staged(t, out=out[i0:i1])
            return out
        return self._lazy('X0', make)

    _X0_BLOCK_BYTES = 1 << 30      # X0 is materialised through device blocks of this size above it

    @X0.setter
    def X0(self, value):
        self._host['X0'] = value                              # gpr.py:379 stores what scale_data returned

    # ------------------------------------------------------------------ a2 scale_data
    _DEVICE_SCALINGS = ('std', 'none', 'pareto', 'vast', 'range', 'level', 'max', 'variance', 'median', 'poisson',
                        'l2-norm')

    def _check_scaling(self, scale_type, axis_cnt):
        known = ['std', 'none', 'pareto', 'vast', 'range', 'level', 'max', 'variance', 'median', 'poisson',
                 'vast_2', 'vast_3', 'vast_4', 'l2-norm']
        if scale_type not in known:
            raise NotImplementedError('The scaling method selected has not been implemented yet')   # :164
        if scale_type not in self._DEVICE_SCALINGS:
            # the reference's own 'vast_2/3/4' branches assign scipy's per-COLUMN kurtosis (an m-vector, :148 / :152 / :156)
            # to a slice of n_points rows: NumPy refuses that assignment with a ValueError unless m == n_points (or
            # m == 1, which broadcasts) -- the same exception here, before any device work
            m = self.X.shape[1]
            if m not in (1, self.n_points):
                raise ValueError(f'could not broadcast input array from shape ({m},) into shape ({self.n_points},)')
            raise NotImplementedError(f"scale_type={scale_type!r} has no device implementation (per-column kurtosis "
                                      'assigned to rows: only defined in the reference when n_points == m); no CPU fallback.')
        # axis_cnt is handed to np.average(x, axis=axis_cnt) on an (n_points, m) block whose result is assigned to n_points rows
        # (:112): 1 and -1 are the row means, None the block mean; 0 / -2 give m column means, which NumPy refuses to put into
        # n_points rows (ValueError) unless the two counts coincide; any other integer is not an axis of a 2-D block (AxisError)
        if axis_cnt is None or axis_cnt == 1 and not isinstance(axis_cnt, bool):
            return axis_cnt
        if isinstance(axis_cnt, (int, np.integer)) and not isinstance(axis_cnt, bool):
            if axis_cnt == -1:
                return 1
            if axis_cnt in (0, -2):
                m = self.X.shape[1]
                if m not in (1, self.n_points):
                    raise ValueError(f'could not broadcast input array from shape ({m},) into shape ({self.n_points},)')
            else:
                raise np.exceptions.AxisError(int(axis_cnt), 2, 'axis')      # (np.average names its argument: 'axis: axis 2 is out of ...')
        raise NotImplementedError(f'axis_cnt={axis_cnt!r}: row centring (1, -1) and scalar centring (None) have a '
                                  'device implementation; no CPU fallback for the rest.')

    def _feature_scale(self, scale_type, cnt, mu, var, m):
        """Per-feature scaling factor (:114-161) from the merged block statistics: cnt rows, block mean mu,
        population variance var of the raw block; 'range' / 'max' add one min/max pass over X."""
        with np.errstate(invalid='ignore', divide='ignore'):
            std = np.sqrt(var)
            if scale_type == 'std':
                return std
            if scale_type == 'none':
                return np.ones_like(std)
            if scale_type == 'pareto':
                return np.sqrt(std)
            if scale_type == 'vast':
                return var / mu
            if scale_type == 'level':
                return mu.copy()
            if scale_type == 'variance':
                return var.copy()
            if scale_type == 'poisson':
                return np.sqrt(mu)
            if scale_type == 'l2-norm':
                return np.sqrt(cnt * m * (var + mu * mu))
            if scale_type == 'median':
                return self._feature_median()
            eng = self._engine()
            mm = self._all_gather(eng.feature_minmax(self._Xd(), self._row0, self.n_points, self.n_features))
            mm = eng.to_host(mm)                              # (world, F, 2)
            fmin, fmax = mm[:, :, 0].min(axis=0), mm[:, :, 1].max(axis=0)
            return fmax - fmin if scale_type == 'range' else fmax

    _SELECT_DIGITS = (13, 13, 13, 13, 12)

    def _feature_median(self):
        """np.median of every raw feature block (:140-141) by radix selection on the device: five histogram passes
        over X (csrc/select.hip), the cumulative walk between passes on the host; histograms are all-reduced so
        every rank follows the same path.  Exact: returns the mean of the two middle order statistics."""
        eng = self._engine()
        Xd = self._Xd()
        F, m = self.n_features, Xd.shape[1]
        N = self.n_points * m                                  # values per feature block (global)
        want = np.array([(N - 1) // 2, N // 2], dtype=np.int64)
        rank = np.tile(want, (F, 1))                           # remaining rank inside the current prefix
        prefix = np.zeros((F, 2), dtype=np.uint64)
        shift = 64
        i64 = eng.torch.int64
        for bits in self._SELECT_DIGITS:
            shift -= bits
            two = bool(np.any(prefix[:, 0] != prefix[:, 1]))
            hist = eng.feature_digit_hist(Xd, self._row0, self.n_points, F, eng.to_device(prefix.view(np.int64), dtype=i64),
                                          shift, bits, two)
            hist = eng.to_host(self._all_reduce(hist))          # (F, 2, 1 << bits)
            cum = np.cumsum(hist, axis=2)
            for f in range(F):
                for t in range(2):
                    b = int(np.searchsorted(cum[f, t], rank[f, t], side='right'))
                    if b >= cum.shape[2]:
                        raise RuntimeError('median selection lost its target (NaN in X?)')
                    rank[f, t] -= cum[f, t, b - 1] if b > 0 else 0
                    prefix[f, t] |= np.uint64(b) << np.uint64(shift)
        sign = np.uint64(1) << np.uint64(63)
        bits_ = np.where(prefix & sign, prefix ^ sign, ~prefix)   # inverse of the order-preserving key
        vals = bits_.view(np.float64)
        return 0.5 * (vals[:, 0] + vals[:, 1])

    def _stats_pass(self, scale_type='std', axis_cnt=1):
        """Fused K1+K3a pass, cross-rank merge, per-feature scale. Leaves rowmean/scale on the device."""
        eng = self._engine()
        Xd = self._Xd()
        F = self.n_features
        tr_ = self._trace = _Trace(eng)
        fused = scale_type if (axis_cnt == 1 and scale_type in getattr(eng, 'SCALE_CODES', ())) else None
        rowmean, gram, fs_d = self._gram_collective(Xd, combine=fused)
        self._merge_stats(gram, fs_d, rowmean, scale_type, axis_cnt)

    def _gram_collective(self, Xd, combine=None):
        """The fused stats + Gram pass over the local rows and the ONE collective of fit(): an all-reduce (sum) of a
        buffer [F m m Gram doubles | world x F x 3 statistics | world first rows], every rank writing its (count, mean, M2)
        triples and its first global row into its own slots and zeros elsewhere, so the sum hands every rank all ranks'
        statistics and row blocks in rank order (adding zeros is exact) -- north_star: a single RCCL all-reduce for the
        Gram matrix.
        Returns rowmean (n_local,), gram (F, m, m) summed over ranks, fstats_all (world, F, 3)."""
        eng = self._engine()
        F, m = self.n_features, Xd.shape[1]
        fill = self._filler_wanted(Xd)
        e0 = eng.timing_event() if fill else None
        if not self._dist():
            rowmean, fstats, gram = eng.stats_gram(Xd, self._row0, self.n_points, F, center=True)
            if fill:
                self._gram_events = (e0, eng.timing_event())
            self._trace.mark('stats_gram')
            return rowmean, gram, fstats[None]
        world, rank = self._world(), self._shard.rank
        self.__dict__.pop('_combined', None)
        nc = self._native_comm()
        if nc is not None and combine is not None and m <= 512 and hasattr(eng, 'fit_gram_pass'):
            # the whole pass -- Gram kernel, finalize, all-reduce, statistics merge + scaled sum -- as ONE call of the library
            # (spr_fit_gram_pass): nothing of the host between the kernels and the collective; combine = the scale_type
            close = self._comm_bracket('allreduce')           # (brackets the whole enqueue here)
            import time
            self.last_comm_ = ('spr_fit_gram_pass (Gram + all_reduce + combine)', (F, m, m), time.time())
            rowmean, buf, packed_d, scale_d, inv_d = eng.fit_gram_pass(Xd, self._row0, self.n_points, F, combine, nc, world)
            close()
            if fill:
                self._gram_events = (e0, eng.timing_event())
            self._trace.mark('stats_gram')
            self._combined = (packed_d, scale_d, inv_d)
            fstats_all = buf[F * m * m:F * m * m + world * F * 3].view(world, F, 3)
            if '_layout' not in self.__dict__:
                self._layout_src = (fstats_all[:, :, 0], buf[F * m * m + world * F * 3:])
            return rowmean, buf[:F * m * m].view(F, m, m), fstats_all
        buf = eng.zeros((F * m * m + world * F * 3 + world,))
        # this rank's first row (exact below 2^53), see _shard_layout -- from a resident scalar: assigning a Python float is a
        # synchronous pageable H2D copy, which queues on an SDMA engine BEHIND the pushes of a p2p field exchange in flight
        # and held the next Gram pass back by their whole duration (profiles/r05_c4share8_p2p_loopback_timeline.txt)
        r0 = self.__dict__.get('_row0_d')                       # (a device tensor: never pickled, see __getstate__)
        if r0 is None:
            r0 = self._row0_d = eng.to_device(np.array([float(self._row0)]))
        buf[F * m * m + world * F * 3 + rank:F * m * m + world * F * 3 + rank + 1].copy_(r0)
        g_view = buf[:F * m * m].view(F, m, m)
        f_view = buf[F * m * m + rank * F * 3:F * m * m + (rank + 1) * F * 3].view(F, 3)
        if getattr(eng, 'supports_gram_out', False):          # the finalize kernel writes straight into the collective buffer
            rowmean, fstats, gram = eng.stats_gram(Xd, self._row0, self.n_points, F, center=True, gram_out=g_view,
                                                   fstats_out=f_view)
        else:                                                 # an engine without the output arguments (the NumPy test double)
            rowmean, fstats, gram = eng.stats_gram(Xd, self._row0, self.n_points, F, center=True)
            g_view.copy_(gram)
            f_view.copy_(fstats)
        if fill:
            self._gram_events = (e0, eng.timing_event())
        self._trace.mark('stats_gram')
        close = self._comm_bracket('allreduce')
        self._all_reduce(buf)
        close()
        fstats_all = buf[F * m * m:F * m * m + world * F * 3].view(world, F, 3)
        if '_layout' not in self.__dict__:
            # rows per (rank, feature) and first rows: the ranks' blocks, carried by the one all-reduce for free
            self._layout_src = (fstats_all[:, :, 0], buf[F * m * m + world * F * 3:])
        return rowmean, buf[:F * m * m].view(F, m, m), fstats_all

    def _filler_wanted(self, Xd):
        import os
        eng = self._engine()
        tr = self.__dict__.get('_trace')
        env = os.environ.get('SPR_GAP_FILLER')
        on = (self.gap_filler or env == '1') and env != '0'
        return bool(on and hasattr(eng, 'gram_filler') and self._GAP_FILL_MIN_M <= Xd.shape[1]
                    and not (tr is not None and tr.on))        # SPR_TRACE synchronises at every mark: its gaps are not fit()'s

    def _queue_gap_filler(self, Xd):
        """Called between the enqueue of the Gram download and the host's wait for it (see gap_filler)."""
        eng = self._engine()
        hist = self.__dict__.get('_gap_hist')
        ev = self.__dict__.pop('_gram_events', None)
        rate = self.__dict__.get('_gram_rows_per_ms')
        self._gap_fill_rows = 0
        self._gram_events_pending = ev
        # A field all-gather left in flight by the previous reconstruct(wait=False) cannot run NEXT TO the Gram or projection
        # workgroups (RCCL's kernel wants 261-280 VGPRs per wave and 19.7 KB of LDS; two Gram waves hold 448 of a SIMD's 512
        # registers, two projection waves all of them): its window is this very gap, so it stays empty
        pf = self.__dict__.get('_pending_field')
        if pf is not None and pf.pending and pf.needs_cus:     # (the p2p exchange runs on the SDMA engines: nothing to leave free)
            return
        if hist and rate and min(hist) >= self._GAP_FILL_MIN_MS:
            # a wide X (m > 256) is filled with the 256-column kernel on its first slice, whose rows cost (256 / m)^2 of what the
            # rows of the whole wide pass -- the rate measured -- cost
            m = Xd.shape[1]
            speed = (m / 256.0) ** 2 if m > 256 else 1.0
            rows = int(self._GAP_FILL_FRACTION * min(hist) * rate * speed) // 4096 * 4096
            rows = min(rows, Xd.shape[0])
            if rows >= 65536:
                eng.gram_filler(Xd, rows, self._row0, self.n_points, self.n_features)
                self._gap_fill_rows = rows

    def _close_gap(self):
        """The projection is about to be launched: record the host gap this fit() had, and the rate of its Gram pass."""
        t0 = self.__dict__.pop('_gap_t0', None)
        if t0 is None:
            return
        import time
        from collections import deque
        eng = self._engine()
        gap_ms = 1e3 * (time.perf_counter() - t0)
        hist = self.__dict__.setdefault('_gap_hist', deque(maxlen=8))
        hist.append(gap_ms)
        ev = self.__dict__.pop('_gram_events_pending', None)
        if ev is not None:
            ms = eng.elapsed_ms(*ev)                     # both events lie in front of the download the host has waited for
            if ms > 0:
                self._gram_rows_per_ms = self._Xd().shape[0] / ms

    def _merge_stats(self, gram, fs_d, rowmean, scale_type, axis_cnt):
        """Per-feature Gram blocks (all-reduced) + per-rank feature statistics -> X_scl per feature and the Gram matrix
        G of X0 = (X - X_cnt)/X_scl (self._G, host)."""
        eng = self._engine()
        Xd = self._Xd()
        m = Xd.shape[1]
        F = self.n_features
        tr_ = self._trace
        if axis_cnt == 1 and scale_type in getattr(eng, 'SCALE_CODES', ()) and hasattr(eng, 'gram_combine'):
            # statistics merge, feature scales and G = sum_f G_f / scl_f^2 on the device (csrc/combine.hip): one
            # download of m^2 + 5F doubles, the scales never leave HBM
            comb = self.__dict__.pop('_combined', None)       # spr_fit_gram_pass has merged already (native communicator)
            packed_d, scale_d, inv_d = comb if comb is not None else eng.gram_combine(gram, fs_d, scale_type)
            fill = self._filler_wanted(Xd) and getattr(self, '_fit_fills_gap', False)

            def gap_hook():
                # the download is enqueued, the host is about to block on it: what goes into the gap behind it -- a
                # reconstruct the caller deferred (useful work), else the filler (discarded work, opt-in)
                if self._flush_deferred():
                    self._gap_fill_rows = 0                    # (the gap holds the deferred launch, not a filler)
                elif fill:
                    self._queue_gap_filler(Xd)
            packed = eng.to_host(packed_d, then=gap_hook)
            if fill:
                import time
                self._gap_t0 = time.perf_counter()
            tr_.mark('collect')
            feat = packed[m * m:].reshape(F, 5)
            self._G = packed[:m * m].reshape(m, m)
            self._scl_f = feat[:, 3].copy()
            self._var_f = self._scl_f ** 2
            self._mu_f = feat[:, 1].copy()
            self._set_precenter_ratio(feat[:, 1], feat[:, 2], feat[:, 4], axis_cnt)
            self._d['rowmean'] = rowmean
            self._d['scale'] = scale_d
            self._d['inv_scale'] = inv_d
            for k in ('X_cnt', 'X_scl', 'X0'):
                self._host.pop(k, None)
            tr_.mark('merge')
            return
        # one download for both: every host round trip is a sync point the GPU idles at
        packed = eng.to_host(eng.torch.cat([gram.reshape(-1), fs_d.reshape(-1)]), then=self._flush_deferred)
        G_f = packed[:gram.numel()].reshape(F, m, m)
        fs = packed[gram.numel():].reshape(fs_d.shape[0], F, 3)
        tr_.mark('collect')
        cnt = np.zeros(F); mu = np.zeros(F); m2 = np.zeros(F)
        for w in range(fs.shape[0]):                         # Chan merge in rank order
            nb, mb, sb = fs[w, :, 0], fs[w, :, 1], fs[w, :, 2]
            tot = cnt + nb
            with np.errstate(invalid='ignore', divide='ignore'):
                d = mb - mu
                frac = np.where(tot > 0, nb / np.where(tot > 0, tot, 1), 0.0)
                m2 = m2 + sb + d * d * cnt * frac
                mu = mu + d * frac
            cnt = tot
        tr = np.trace(G_f, axis1=1, axis2=2)
        # a feature WITHOUT rows -- only possible in a partial row group (RowShard(partial=True): one rank's block of a
        # larger job run alone) -- takes no part: scale 1, and its Gram block is zero anyway
        present = cnt > 0
        with np.errstate(invalid='ignore', divide='ignore'):
            var_f = np.where(present, (tr + m * m2) / np.where(present, cnt * m, 1.0), 0.0)   # population variance (:115)
        scl = self._feature_scale(scale_type, cnt, mu, var_f, m)
        self._scl_f = np.where(present, scl, 1.0)
        self._var_f = self._scl_f ** 2                        # what the Gram blocks are divided by
        self._mu_f = mu.copy()
        with np.errstate(invalid='ignore', divide='ignore'):
            fluct = np.where(present, tr / np.where(present, cnt * m, 1.0), 0.0)
        self._set_precenter_ratio(mu, var_f, fluct, axis_cnt)
        if axis_cnt is None:
            # scalar centre per feature (:112 with axis=None): turn the row-centred Gram blocks into those
            # of (X - mu_f) with the two column-sum vectors, and make X_cnt the per-feature constant
            cs = eng.to_host(self._all_reduce(eng.colsums(Xd, self._row0, self.n_points, F, rowmean)))
            v = cs[:, 1, :] - mu[:, None] * cs[:, 0, :]       # sum_i (mean_i - mu_f) c_i
            G_f = G_f + v[:, :, None] + v[:, None, :] + m2[:, None, None]
            rowmean = eng.fill_feature(Xd.shape[0], self._row0, self.n_points, eng.to_device(mu))
        with np.errstate(invalid='ignore', divide='ignore'):
            self._G = np.sum(G_f / self._var_f[:, None, None], axis=0)   # Gram matrix of X0 = (X - X_cnt)/X_scl
        self._d['rowmean'] = rowmean
        self._d['scale'] = eng.to_device(self._scl_f)
        with np.errstate(divide='ignore'):
            self._d['inv_scale'] = eng.to_device(1.0 / self._scl_f)
        for k in ('X_cnt', 'X_scl', 'X0'):
            self._host.pop(k, None)
        tr_.mark('merge')

    # The projection kernels remove the row mean in their epilogue, x.W - mean (1^T W): the products carry the mean
    # through the MFMA and lose log10(|mean| / |x - mean|) digits, which W = V/S amplifies by sigma_1/sigma_i for the
    # small modes.  Above this product the mean is subtracted from the operand before the multiplication instead
    # (spr_project_stream_* centre mode 2) -- the reference's own order of operations (:169).
    _PRECENTER_ABOVE = 1e6

    def _set_precenter_ratio(self, mu, var, fluct, axis_cnt):
        """Per feature: how large the centre the projection's epilogue has to cancel is, relative to what is left after the
        cancellation.  Row centring (axis_cnt = 1): the rows' own means -- the block mean plus four standard deviations
        of the row means, sqrt(var - fluct), as a stand-in for max_i |mean_i| -- over the rms of the row-centred values,
        sqrt(fluct) = sqrt(trace(G_f) / (count m)): the block std would not do, it contains the spread of the means.
        Scalar centring (axis_cnt = None): X_cnt is the block mean itself and what remains is the whole block's spread."""
        mu, var, fluct = (np.asarray(a, dtype=np.float64) for a in (mu, var, fluct))
        with np.errstate(invalid='ignore', divide='ignore'):
            if axis_cnt is None:
                self._pc_ratio = np.abs(mu) / np.sqrt(var)
            else:
                self._pc_ratio = (np.abs(mu) + 4.0 * np.sqrt(np.maximum(var - fluct, 0.0))) / np.sqrt(fluct)

    def _needs_precenter(self, kappa):
        ratio = getattr(self, '_pc_ratio', None)
        if ratio is None or not np.isfinite(kappa):
            return False
        ratio = ratio[np.isfinite(ratio)]
        return bool(ratio.size and ratio.max() * kappa > self._PRECENTER_ABOVE)

    def scale_data(self, scale_type='std', axis_cnt=1):
        """Reference :83-171.  Sets X_cnt / X_scl and returns the scaled matrix X0."""
        self._flush_deferred()
        axis_cnt = self._check_scaling(scale_type, axis_cnt)
        self._stats_pass(scale_type, axis_cnt)
        return self.X0

    def scale_limits(self, limits):
        """Reference :173-210 (the method GPR users call on the base class, tests/test_gpr_data.py:95): per-feature
        limits -> per-row scaled limits [(limit_f - X_cnt)/X_scl], with the reference's +-1000 block clamps.
        Host arithmetic on the (n_local,) centring vector; X_scl is one scalar per feature."""
        X_cnt = self.X_cnt[:, 0]
        feat = self._feature_rows()
        out = []
        for limit in limits:
            limit = np.asarray(limit, dtype=np.float64)
            limit0 = (limit[feat] - X_cnt) / self._scl_f[feat]
            for f in range(self.n_features):                  # :200-203, per feature block (local rows of it)
                sel = feat == f
                if sel.any():
                    if limit0[sel].min() < -1000:
                        limit0[sel] = -1000
                    elif limit0[sel].max() > 1000:
                        limit0[sel] = 1000
            out.append(limit0)
        return out

    def _csr_device(self, C, known=None):
        """(indptr, indices, vals) device tensors of a dense / scipy.sparse matrix with n columns."""
        import scipy.sparse as sp
        eng = self._engine()
        if known is not None:
            indptr, indices, vals = known
        elif isinstance(C, DeviceCSR):                        # already in HBM, rows sorted (camera.project(to_host=False))
            return C.tensors(eng)
        elif isinstance(C, OneHotRows):
            if C.ndim != 2:
                raise ValueError('a measurement matrix has two dimensions')
            indptr, indices, vals = np.arange(C.shape[0] + 1), C.rows, np.ones(C.shape[0])
        else:
            Cs = C.tocsr() if sp.issparse(C) else sp.csr_matrix(np.asarray(C, dtype=np.float64))
            Cs.sort_indices()
            indptr, indices, vals = Cs.indptr, Cs.indices, Cs.data
        t = eng.torch
        return (eng.to_device(indptr, dtype=t.int64), eng.to_device(indices, dtype=t.int64), eng.to_device(vals))

    def _sampled(self, sampling, matmul=False):
        """S.Ur, S.X_cnt, S.X_scl for a sampling matrix S (s, n) -- reference :233, :366."""
        if sampling.shape[1] != self._n_global:
            # NumPy's own text, as the reference's first product with S raises it: sampling.dot(X_cnt) in reconstruct (:366-368),
            # sampling @ X_cnt in unscale_data (:233)
            n, c = self._n_global, sampling.shape[1]
            if matmul:
                raise ValueError('matmul: Input operand 1 has a mismatch in its core dimension 0, with gufunc signature '
                                 f'(n?,k),(k,m?)->(n?,m?) (size {n} is different from {c})')
            raise ValueError(f'shapes ({sampling.shape[0]},{c}) and ({n},1) not aligned: {c} (dim 1) != {n} (dim 0)')
        eng = self._engine()
        ip, ix, v = self._csr_device(sampling)
        # unscale_data reads X_scl and X_cnt only (:233): after scale_data() alone there is no basis yet, and none is needed
        Ur_d = None if matmul and 'Ur' not in self._d else self._fitted('Ur', 'Ur')
        Th, cnt, scl = eng.measure_csr(ip, ix, v, Ur_d, self._row0, self._fitted('rowmean', 'X_scl' if matmul else 'X_cnt'),
                                       scale=self._d['scale'], n_points=self.n_points)
        return (None if Th is None else self._all_reduce(Th)), self._all_reduce(cnt), self._all_reduce(scl)

    # ------------------------------------------------------------------ a11 unscale_data
    def unscale_data(self, x0, sampling=None):
        """Reference :212-240: x = X_scl * x0 + X_cnt for an (n_local,) vector, or with ``sampling`` (s, n)
        x = (S X_scl) * x0 + S X_cnt for an (s,) vector."""
        self._flush_deferred()
        if type(x0) is not np.ndarray:
            raise NotImplementedError('unscale_data of a cvxpy expression is outside the device path.')
        eng = self._engine()
        if sampling is not None:
            _, cnt, scl = self._sampled(sampling, matmul=True)
            ones = eng.to_device(np.ones(1))
            t = eng.unscale(eng.to_device(x0), 0, x0.shape[0], 1, cnt, ones, rowscale=scl)
        else:
            t = eng.unscale(eng.to_device(x0), self._row0, self.n_points, self.n_features,
                            self._fitted('rowmean', 'X_scl'), self._d['scale'])        # (:235 reads X_scl first)
        return eng.to_host(t)

    # ------------------------------------------------------------------ a4 reduction
    def _select_rank(self, exp_variance, n_cols, select_modes, n_modes):
        """Integer logic of ROM.reduction (:314-333), same exceptions."""
        if select_modes == 'variance':
            if not 0 <= n_modes <= 100:
                raise ValueError('The parameter n_modes is outside the[0-100] range.')
            if n_modes == 100:
                r = n_cols
            else:
                r = 1
                while exp_variance[r - 1] < n_modes:
                    r += 1
        elif select_modes == 'number':
            if not type(n_modes) is int:
                raise TypeError('The parameter n_modes is not an integer.')
            if not 1 <= n_modes <= n_cols:
                raise ValueError('The parameter n_modes is outside the [1-m] range.')
            r = n_modes
        else:
            raise ValueError('The select_mode value is wrong.')
        return r

    def reduction(self, U, A, exp_variance, select_modes, n_modes):
        """Reference :281-340 (host arrays in, views out)."""
        r = self._select_rank(exp_variance, A.shape[1], select_modes, n_modes)
        self.r = r
        return U[:, :r], A[:, :r]

    # ------------------------------------------------------------------ a3 decomposition
    @staticmethod
    def _expvar(lam):
        lam_pos = np.maximum(lam, 0.0)
        return 100 * np.cumsum(lam_pos) / np.sum(lam_pos)      # :274-275

    def _eig_local(self, G, rank_of):
        """This rank's eigen-solve of the (m, m) Gram matrix -> (lam descending (m,), V with r or m columns, unsigned).
        The top-r route (dsytrd + dsterf + r inverse iterations + dormqr) for m >= 96 when the caller only needs r <= m/2
        vectors and sigma_1/sigma_r is within the plain Gram route's range (the refinement pass needs all of V)."""
        m = G.shape[0]
        if (rank_of is not None and _eigen._EIGH_TOP_NATIVE_MIN_M <= m < _eigen._EIGH_TOP_MIN_M
                and getattr(rank_of, 'known_r', None) is not None):
            # the number of modes is given (select_modes='number'): the whole route in one library call
            r = rank_of.known_r
            if 2 * r <= m:
                got = _eigen._eig_top_native(G, r)
                if got is not None and np.isfinite(got[0][0]) and not np.sqrt(max(got[0][r - 1], 0.0)) * _GRAM_KAPPA_REFINE < np.sqrt(max(got[0][0], 0.0)):
                    return got
        if rank_of is not None and m >= _eigen._EIGH_TOP_MIN_M:
            lam_a, fac = _eigen._eigh_tridiagonal(G)
            lam = lam_a[::-1].copy()
            S = np.sqrt(np.maximum(lam, 0.0))
            r = rank_of(self._expvar(lam))
            if 2 * r <= m and np.isfinite(S[0]) and not S[r - 1] * _GRAM_KAPPA_REFINE < S[0]:
                V = _eigen._eigvecs_top(fac, lam_a, r)
                if V is not None:
                    return lam, V
        lam, V = _eigen._eigh_small(G)
        return lam[::-1].copy(), np.ascontiguousarray(V[:, ::-1])

    def _spectrum(self, G, rank_of=None):
        """Eigen-decomposition of the (m,m) Gram matrix -> S (desc), V, explained variance (:272-275).
        ``rank_of(exp_variance) -> r``: the caller only needs the r leading vectors -- V then has r columns whenever
        the top-r route applies (_eig_local) and all m otherwise.
        Sharded: every rank solves for itself (identical bits in, identical bits out on one node: no exchange), checked
        ONCE per object by a digest all-gather at the first fit(); if the ranks differ -- or with
        RowShard(broadcast_basis=True) -- only rank 0 solves and its factors are broadcast in one fixed-size message
        [route, columns, lam (m), V (m x m, padded)], so that no rank-local decision (the route, r, a failed inverse
        iteration) can change the size or the branch of a collective."""
        if not np.all(np.isfinite(G)):
            # a constant feature (X_scl = 0 -> X0 = nan/inf, :169) or a NaN/Inf in X: np.linalg.svd(X0) (:272) raises
            raise np.linalg.LinAlgError('SVD did not converge')
        m = G.shape[0]
        if self._broadcasts_basis():
            lam, V = self._broadcast_factors(G, rank_of, None)
        else:
            lam, V = self._eig_local(G, rank_of)
            if self._dist() and not self.__dict__.get('_basis_checked', False):
                self._basis_checked = True
                if not self._factors_agree(lam, V):
                    import sys
                    self._basis_diverged = True
                    if self._shard.rank == 0:
                        print('[openmeasure_amd] the ranks\' host eigen-solves of the same Gram matrix differ (hosts or LAPACK '
                              'builds differ): rank 0\'s factors are broadcast from now on', file=sys.stderr)
                    lam, V = self._broadcast_factors(G, rank_of, (lam, V))
        self.basis_broadcast_ = bool(self._broadcasts_basis())
        return np.sqrt(np.maximum(lam, 0.0)), _eigen._sign_fix(V), self._expvar(lam)

    def _refine_spectrum(self, S, V, r, Xd, row0, n_points, n_features, inv_scale_d, rowmean_d, center, rank_of=None):
        """Conditioning safeguard of the Gram route (hard part 1).

        The eigenvectors of G = X0^T X0 carry an error eps * (sigma_1/sigma_i)^2, which LAPACK's SVD of X0 itself
        (reference :272) does not have.  One more pass over X removes it: with the first-stage factors V^, S^,
        Y = X0 V^ diag(1/S^) has columns of nearly unit norm that are nearly orthogonal, so its Gram matrix
        H = Y^T Y (same MFMA kernels: projection of a row block into an f64 scratch block, Gram of the block) is
        formed with errors relative to 1, not to sigma_1^2 -- the small modes are now resolved to eps * sigma_1/sigma_i
        like in the reference.  From H = Z L Z^T:  X0 = (Y Z L^-1/2) (L^1/2 Z^T diag(S^) V^T) = Q M with Q
        orthonormal, and the SVD of the m x m matrix M gives the singular values and right singular vectors of X0.
        Repeated (at most _GRAM_REFINE_MAX_PASSES passes) until the retained block of H is well conditioned;
        raises LinAlgError if it never is -- never returns silently degraded sensors.
        ``rank_of``: exp_variance -> number of modes the caller will keep (so that the last pass may compute only that many
        right singular vectors; columns r .. m of the V returned are zero then).
        Returns (S, V, exp_variance, passes)."""
        eng = self._engine()
        n_loc, m = Xd.shape
        eps = np.finfo(float).eps
        # row blocks of the f64 scratch matrix Y: up to 8 GiB (a quarter of what is free), equal in size, so that a pass over 9M
        # rows is 3 projection + Gram launch pairs instead of 9 (each pair has its ramp and tail; one 18 GB block measured no
        # better than three of 6 GB, and its allocation now and then cost 5 ms)
        budget = 1 << 31
        try:
            free = eng.torch.cuda.mem_get_info(eng.device)[0] if hasattr(eng, 'device') and eng.device.type == 'cuda' else 0
            budget = int(min(8 << 30, max(1 << 31, free // 4)))
        except (RuntimeError, AttributeError):
            pass
        block = int(max(1 << 16, min(n_loc, budget // (8 * (m + (m & 1))))))
        n_blocks = -(-n_loc // block)
        block = -(-n_loc // n_blocks)                         # equal blocks: no short last pair of launches (ramp and tail for little work)
        block = min(n_loc, -(-block // 16) * 16)
        Y = eng.empty((min(block, n_loc), m + (m & 1)))
        passes = 0
        import time
        prof = self.refine_profile_ = dict(device_ms=0.0, host_ms=0.0)
        while True:
            passes += 1
            t_a = time.perf_counter()
            floor = S[0] * np.sqrt(m * eps)
            d = np.maximum(S, floor if floor > 0 else 1.0)
            W2 = eng.to_device(V / d)
            pre = bool(center and self._needs_precenter(S[0] / d[r - 1]))
            H_d = None
            for i0 in range(0, n_loc, block):
                rows = min(block, n_loc - i0)
                eng.project_f64(Xd, i0, rows, row0, n_points, n_features, inv_scale_d, W2, rowmean_d, Y, center=center,
                                precenter=pre)
                Yb = Y[:rows, :m] if Y.shape[1] != m else Y[:rows]
                _, _, g = eng.stats_gram(Yb, 0, rows, 1, center=False)
                H_d = g[0].clone() if H_d is None else H_d.add_(g[0])
            H = eng.to_host(self._all_reduce(H_d))
            t_b = time.perf_counter()
            H = 0.5 * (H + H.T)
            # X0 = Q M with Q orthonormal: from the Cholesky factor H = R^T R (Q = Y R^-1, M = R diag(d) V^T: 0.3 ms at
            # m = 256 against 2.7 ms for the eigen-decomposition H = Z L Z^T, M = L^1/2 Z^T diag(d) V^T, which remains the
            # route when H is not numerically positive definite -- a first stage too far off, the null mode of a full-rank fit)
            with _eigen._one_blas_thread():                           # m x m: a many-core BLAS pool only gets in the way
                from scipy.linalg import lapack
                Rc, info = lapack.dpotrf(H, lower=0, clean=1)
                if info == 0 and np.all(np.isfinite(Rc)) and Rc.diagonal().min() > 1e-7 * Rc.diagonal().max():
                    t_c = time.perf_counter()
                    B = Rc * d[None, :]
                else:
                    lamH, Z = _eigen._eigh_small(H)
                    t_c = time.perf_counter()
                    B = (np.sqrt(np.maximum(lamH, 0.0))[:, None] * Z.T) * d[None, :]
                # M = B V^T, V orthogonal: the singular values of M are B's, its right singular vectors V times B's
                t_d = time.perf_counter()
                # of this SVD only the singular values and the r retained right vectors are used once the pass has converged
                # (the usual case): the one-call route computes exactly those (0.65 of dgesdd's time at m = 256, r = 64);
                # rows r .. m of Vt stay zero then.  A pass that has NOT converged needs all of V for the next one (below).
                # (not when the ranks take rank 0's factors: the route must not depend on a rank-local outcome there)
                part = None if self._broadcasts_basis() else _eigen._svd_top_native(B, r)
                if part is not None:
                    S_new = part[0]
                    Vt = np.zeros((m, m))
                    Vt[:r] = (V @ part[1]).T                    # m x m x r instead of forming M (m x m x m)
                else:
                    M = B @ V.T
                    _, S_new, Vt = np.linalg.svd(M)
            t_e = time.perf_counter()
            prof['eigh_ms'] = prof.get('eigh_ms', 0.0) + 1e3 * (t_c - t_b)
            prof['M_ms'] = prof.get('M_ms', 0.0) + 1e3 * (t_d - t_c)
            prof['svd_ms'] = prof.get('svd_ms', 0.0) + 1e3 * (t_e - t_d)
            S_new, Vt = self._same_on_all_ranks(S_new, Vt)
            prof['device_ms'] += 1e3 * (t_b - t_a)
            # is the pass converged?  The retained columns of Y must have come out nearly orthonormal.  Modes below
            # 1e-12 sigma_1 (the null mode that row-centring creates when all m modes are kept) are rounding noise
            # in the reference as well and are left out of the verdict.
            keep = np.flatnonzero(S_new[:r] > 1e-12 * S_new[0])
            dn = np.sqrt(np.maximum(np.diag(H), np.finfo(float).tiny))
            Hk = (H[np.ix_(keep, keep)] / dn[keep, None]) / dn[None, keep]     # unit diagonal
            rho = float(np.max(np.sum(np.abs(Hk), axis=1) - np.abs(np.diag(Hk)))) if len(keep) else 0.0
            if rho < 0.5 and np.all(np.isfinite(Hk)):
                # Gershgorin: the eigenvalues of the retained block lie in [1 - rho, 1 + rho] -- condition below 3 without solving
                # for them (the usual case: off-diagonals of 1e-3)
                cond_r = (1.0 + rho) / (1.0 - rho)
            else:
                with _eigen._one_blas_thread():
                    ev = np.linalg.eigvalsh(Hk)
                cond_r = ev[-1] / max(ev[0], np.finfo(float).tiny)
            converged = cond_r < 4.0                           # |off-diagonal| of the retained block well below 1
            if part is not None and (not converged or (rank_of is not None and rank_of(self._expvar(S_new * S_new)) > r)):
                # all of V is needed after all: another pass follows, or the refined spectrum asks for more modes than were kept
                with _eigen._one_blas_thread():
                    _, S_new, Vt = np.linalg.svd(B @ V.T)
            S, V = S_new, _eigen._sign_fix(Vt.T.copy())
            prof['host_ms'] += 1e3 * (time.perf_counter() - t_b)
            if converged:
                break
            if passes >= _GRAM_REFINE_MAX_PASSES:
                raise np.linalg.LinAlgError(
                    f'fit: sigma_1/sigma_r = {S[0] / max(S[r - 1], np.finfo(float).tiny):.3g} is beyond what the Gram '
                    f'route resolves even after {passes} refinement passes (retained block of the second-stage Gram '
                    f'matrix still has condition {cond_r:.3g}); keep fewer modes or rescale the data.')
        lam = S * S
        exp_variance = 100 * np.cumsum(lam) / np.sum(lam)
        return S, V, exp_variance, passes

    def _basis_from_gram(self, G, select_modes, n_modes, center, inv_scale_d, may_defer=False):
        """``may_defer`` (fit() only): the projection may be recorded instead of launched (defer_project); Ur_d is then None."""
        eng = self._engine()
        Xd = self._Xd()
        m = Xd.shape[1]
        import time
        t_eig = time.perf_counter()
        def rank_of(ev):
            return self._select_rank(ev, m, select_modes, n_modes)
        # select_modes='number': r is known before the eigenvalues are (the one-call top-r route, _eigen._eig_top_native)
        rank_of.known_r = n_modes if (select_modes == 'number' and type(n_modes) is int and 1 <= n_modes <= m) else None
        S, V, exp_variance = self._spectrum(G, rank_of)
        self.eig_ms_ = 1e3 * (time.perf_counter() - t_eig)      # host wall time of the m x m eigen-solve (bench.py: per rank)
        self._trace.mark('eigh')
        r = self._select_rank(exp_variance, m, select_modes, n_modes)
        self.gram_refine_passes_ = 0
        if S[r - 1] * _GRAM_KAPPA_REFINE < S[0]:
            import time
            t_ref = time.perf_counter()
            S, V, exp_variance, self.gram_refine_passes_ = self._refine_spectrum(
                S, V, r, Xd, self._row0, self.n_points, self.n_features, inv_scale_d, self._d.get('rowmean'), center,
                rank_of=rank_of)
            r = self._select_rank(exp_variance, m, select_modes, n_modes)
            self.refine_ms_ = 1e3 * (time.perf_counter() - t_ref)      # host wall time of the refinement (it synchronises)
            self._trace.mark('refine')
        # modes below sqrt(m eps) sigma_1 carry no information on the Gram route; keep the
        # projection finite for them (their reference counterparts are LAPACK rounding noise)
        floor = S[0] * np.sqrt(m * np.finfo(float).eps) if not self.gram_refine_passes_ else S[0] * m * np.finfo(float).eps
        S_safe = np.maximum(S[:r], floor if floor > 0 else 1.0)
        W = V[:, :r] / S_safe
        self._trace.mark('W')
        # (W's previous reader is the projection of the previous fit(), in front of the Gram download the host has waited for)
        W_d = eng.upload_reuse(('W', id(self)), W) if hasattr(eng, 'upload_reuse') else eng.to_device(W)
        self._trace.mark('upload')
        self.precentered_ = bool(center and self._needs_precenter(S[0] / S_safe[-1]))
        nrm0 = self._norms_buffer(Xd, r, self.precentered_ and center)
        kw = {} if nrm0 is None else {'norms': nrm0}
        self._close_gap()
        self._flush_deferred()                                # (normally done in the gap already: see _merge_stats)
        args = (Xd, self._row0, self.n_points, self.n_features, inv_scale_d, W_d)
        out = self._d.pop('Ur', None)
        spare = self.__dict__.pop('_ur_spare', None)          # (the buffer of a projection that was recorded and discarded)
        kw.update(center=center, out=out if out is not None else spare, rowmean=self._d.get('rowmean'),
                  basis_dtype=self._basis_dtype(), precenter=self.precentered_)
        # defer_project: the plain single-device projection with W resident in LDS (no refinement pass, no pre-centring) is
        # only RECORDED; an engine that cannot emit the field from it defers all the same (its launch is then always plain)
        can_fuse = getattr(eng, 'project_field_max', None)
        if (may_defer and center and self._defers_project() and not self._dist() and self._shard is None
                and not self.precentered_ and not self.gram_refine_passes_ and m <= 256 and r <= 64
                and (can_fuse is None or can_fuse(Xd, r) > 0)):
            self._proj_pending = dict(args=args, kw=kw, r=r, nf=0 if can_fuse is None else int(can_fuse(Xd, r)))
            self._d.promised = ('Ur',) if nrm0 is None else ('Ur', 'nrm0')
            import weakref
            me = weakref.ref(self)                            # (no cycle object -> state -> object: results and HBM are
            self._d.guard = lambda: me()._flush_project()     #  released when the last reference goes, not at the next gc)
            Ur_d = None
        else:
            Ur_d = eng.project(*args, **kw)
            if nrm0 is not None:
                self._d['nrm0'] = nrm0
        self._trace.mark('project')
        Ar = V[:, :r] * S[:r]                                # A = (diag(S) Vt).T  (:273)
        return Ur_d, Ar, exp_variance[:r], S, r, V[:, :r]

    def decomposition(self, X0, select_modes='variance', n_modes=99):
        """Reference :242-279 on a caller-supplied scaled matrix X0 (host ndarray, local rows).
        Returns (Ur, Ar, exp_variance[:r]) as host arrays.  When X0 is the very array scale_data() returned
        (the pattern of GPR.fit, gpr.py:379-381) the Gram blocks of that pass and the resident X are used instead
        of uploading X0 and reading it twice."""
        self._flush_deferred()
        eng = self._engine()
        if X0 is self._host.get('X0') and '_G' in self.__dict__ and 'rowmean' in self._d:
            G = self._G
            self._trace = _Trace(eng)
            self._d.pop('Ur', None)
            self._d.pop('nrm0', None)
            Ur_d, Ar, expv, _, r, _ = self._basis_from_gram(G, select_modes, n_modes, True, self._d['inv_scale'])
        else:
            X0d = eng.to_device(X0)
            _, _, gram = eng.stats_gram(X0d, 0, X0d.shape[0], 1, center=False)
            G = eng.to_host(self._all_reduce(gram))[0]
            ones = eng.to_device(np.ones(1))
            m = X0d.shape[1]
            S, V, exp_variance = self._spectrum(G, lambda ev: self._select_rank(ev, m, select_modes, n_modes))
            r = self._select_rank(exp_variance, m, select_modes, n_modes)
            floor = S[0] * np.sqrt(m * np.finfo(float).eps)
            if S[r - 1] * _GRAM_KAPPA_REFINE < S[0]:
                S, V, exp_variance, _ = self._refine_spectrum(S, V, r, X0d, 0, X0d.shape[0], 1, ones, None, False,
                                                              rank_of=lambda ev: self._select_rank(ev, m, select_modes, n_modes))
                r = self._select_rank(exp_variance, m, select_modes, n_modes)
                floor = S[0] * m * np.finfo(float).eps
            W = V[:, :r] / np.maximum(S[:r], floor if floor > 0 else 1.0)
            Ur_d = eng.project(X0d, 0, X0d.shape[0], 1, ones, eng.to_device(W), center=False)
            Ar, expv = V[:, :r] * S[:r], exp_variance[:r]
        self.r = r
        Ur = np.ascontiguousarray(eng.to_host(Ur_d))
        self._last_decomp = (Ur, Ur_d)
        return Ur, Ar, expv

    # ------------------------------------------------------------------ a5 fit
    def fit(self, scale_type='std', axis_cnt=1, select_modes='variance', n_modes=99, basis=None):
        """Reference :463-511."""
        axis_cnt = self._check_scaling(scale_type, axis_cnt)
        if basis is None and select_modes not in ('variance', 'number'):
            raise ValueError('The select_mode value is wrong.')
        eng = self._engine()
        self._drop_project()                                  # a projection still recorded wrote a basis this call replaces
        self.scale_type = scale_type
        for k in ROM._LAZY + ('C', 'Theta', '_pending', '_cpod_Ar0', '_pf_E_tot', 'n_seen_', 'partial_fit_info_'):
            self.__dict__.pop(k, None)                        # (the last three: partial_fit's; fit() starts over from X)
        # CPOD relies on Ur^T Ur = I and Ar = (Ur^T X0)^T: true of the basis this call computes, in f64 storage
        if basis is not None:
            self._basis_foreign = 'fit(basis=...) took the basis from the caller'
        elif str(self._basis_dtype()) == 'torch.float32':
            self._basis_foreign = "DeviceMatrix(basis='f32') stores the basis in float32: orthonormal to f32 rounding only"
        else:
            self._basis_foreign = None
        for k in ('cnt', 'Theta', 'nrm0'):                    # a new basis invalidates the trained measurement state
            self._d.pop(k, None)
        took = self._device_fit(scale_type, axis_cnt, select_modes, n_modes, basis)
        if took is True:
            return
        if took != 'merged':                                  # 'merged': the device route left its statistics behind
            self._fit_fills_gap = basis is None               # the host eigen-solve follows: see gap_filler
            try:
                self._stats_pass(scale_type, axis_cnt)
            finally:
                self._fit_fills_gap = False
        self._host.clear()
        if basis is None:
            Ur_d, Ar, expv, S, r, V_r = self._basis_from_gram(self._G, select_modes, n_modes, True, self._d['inv_scale'],
                                                              may_defer=True)
            self.exp_variance_ = expv
            self.S_ = S
        else:
            self._flush_deferred()
            Ur_d = eng.to_device(basis[0])
            Ar = np.asarray(basis[1])
            V_r = None
        if Ur_d is not None:                                  # (None: the projection was recorded, defer_project)
            self._d['Ur'] = Ur_d
        if '_layout_src' in self.__dict__ and '_layout' not in self.__dict__:
            # first sharded fit(): the table of row blocks rode on the all-reduce -- check now that the blocks tile the global
            # rows (ValueError on every rank), not at the first gather: placement, train and predict use global indices too
            self._shard_layout(Ur_d.shape[0])
        self.Ar = Ar
        self.r = Ar.shape[1]
        Sigma_r = np.linalg.norm(Ar, axis=0)                  # :504-508
        self.Sigma_r = Sigma_r
        if V_r is not None:
            self.Vr = V_r * (np.linalg.norm(V_r, axis=0) ** -1)   # = Ar / Sigma_r, also when a sigma underflowed to 0
        else:
            self.Vr = Ar / Sigma_r
        self._trace.report()

    def _device_fit(self, scale_type, axis_cnt, select_modes, n_modes, basis):
        """fit() without any host synchronisation: statistics merge, feature scales, eigen-decomposition
        (Jacobi, csrc/spectrum.hip) and W = V_r S_r^-1 all stay on the device.  Taken when the spectrum fits one
        workgroup and beats the host round trip (m <= 24), the number of modes is given, and the scaling derives
        from block mean/variance;
        Ar, Sigma_r, Vr, exp_variance_, X_scl are copied to the host on first access."""
        eng = self._engine()
        if basis is not None or select_modes != 'number' or axis_cnt != 1 or not hasattr(eng, 'spectrum'):
            return False
        if scale_type not in eng.SCALE_CODES:
            return False
        Xd = self._Xd()
        m = Xd.shape[1]
        if m > min(eng.spectrum_max_m, _DEVICE_SPECTRUM_MAX_M):
            return False
        r = self._select_rank(None, m, 'number', n_modes)      # same TypeError / ValueError as the reference
        F = self.n_features
        tr_ = self._trace = _Trace(eng)
        rowmean, gram, fs_all = self._gram_collective(Xd)
        sp = eng.spectrum(gram, fs_all, scale_type, r)
        tr_.mark('stats_gram+spectrum')
        self._host.clear()
        self._d['rowmean'] = rowmean
        self._d['scale'] = sp['scale']
        self._d['inv_scale'] = sp['inv_scale']
        nrm0 = self._norms_buffer(Xd, r)
        kw = {} if nrm0 is None else {'norms': nrm0}
        self._flush_deferred()
        self._d['Ur'] = eng.project(Xd, self._row0, self.n_points, F, sp['inv_scale'], sp['W'], center=True,
                                    out=self._d.pop('Ur', None), rowmean=rowmean, basis_dtype=self._basis_dtype(), **kw)
        if nrm0 is not None:
            self._d['nrm0'] = nrm0
        tr_.mark('project')
        # the only download of this path: the two singular values that decide whether the Gram route was good enough,
        # the Jacobi verdict (sweeps, off^2, diag^2) and the feature statistics -- fetched after the projection has been
        # enqueued, so the device never idles on the good path
        chk = eng.to_host(eng.torch.cat([sp['S'][:1], sp['S'][r - 1:r], sp['info'], sp['feat'].reshape(-1)]))
        feat = chk[5:].reshape(F, 5)
        self._scl_f, self._mu_f = feat[:, 3].copy(), feat[:, 1].copy()
        self._set_precenter_ratio(feat[:, 1], feat[:, 2], feat[:, 4], axis_cnt)
        good = bool(np.all(np.isfinite(chk)))
        if good:
            converged = chk[2] < eng.spectrum_max_sweeps or chk[3] <= 1e-24 * chk[4]
            kappa = chk[0] / chk[1] if chk[1] > 0 else np.inf
            good = converged and not kappa > _GRAM_KAPPA_REFINE and not self._needs_precenter(kappa)
        if not good:
            # out of the plain Gram route's range (or non-finite data): the host route decides -- refinement pass,
            # pre-centred projection or LinAlgError -- from the Gram blocks this pass already has (no second read of X)
            self._merge_stats(gram, fs_all, rowmean, scale_type, axis_cnt)
            self._device_fit_fallback_ = True
            return 'merged'
        self.r = r
        self.gram_refine_passes_ = 0
        self.precentered_ = False
        sp['r'] = r
        self._pending = sp
        tr_.report()
        return True

    # ------------------------------------------------------------------ a10 reconstruct
    def reconstruct(self, Ar, sampling=None, to_host=True, wait=True):
        """Reference :342-375.  Returns X_rec of shape (n, n_p) (all ranks' rows, gathered).

        ``to_host=False`` returns the device tensor of shape (n_p, n) instead (same values,
        column-major) and skips the PCIe copy.  With ``wait=False`` as well, a PendingField comes back
        right after the all-gather of the field has been ENQUEUED, so the gather (720 MB per rank at config 4)
        runs on the communication stream under whatever the caller launches next -- e.g. the MFMA-bound Gram
        pass of the next fit(); call ``.wait()`` before reading it.  (With ``defer_reconstruct``, the default, that form only
        RECORDS its launch: see the attribute.)"""
        eng = self._engine()
        self._flush_deferred(project=False)                   # an earlier deferred launch keeps its place in the order
        defer = sampling is None and self._defers() and not to_host and not wait
        # defer_reconstruct records the launch: a caller's own tensor is cloned -- what it holds NOW (n_p x r doubles),
        # whatever the caller writes into it before the launch
        A_d = self._coefficients(eng, Ar, own=defer)
        if A_d.shape[0] == 0:                                 # no measurement vectors: (n, 0), nothing to launch
            rows = self._n_global if sampling is None else sampling.shape[0]
            return np.zeros((rows, 0)) if to_host else eng.empty((0, rows))
        if sampling is not None:                              # :365-368 -- (S Ur) Ar^T, un-scaled with S X_scl, S X_cnt
            Th, cnt, scl = self._sampled(sampling)
            ones = eng.to_device(np.ones(1))
            Thp = Th if Th.shape[1] % 2 == 0 else eng.torch.nn.functional.pad(Th, (0, 1))[:, :Th.shape[1]]
            out = eng.reconstruct(Thp, 0, Th.shape[0], 1, cnt, ones, A_d, rowscale=scl)
            return out if not to_host else eng.to_host(out, result=True).T
        rec = self.__dict__.get('_proj_pending')
        if (rec is not None and A_d.shape[0] <= rec['nf'] and A_d.shape[1] == rec['r'] and A_d.dtype == eng.torch.float64
                and 'rowmean' in self._d):
            # defer_project: fit() recorded its projection, and this is the call it waited for -- ONE kernel writes the basis
            # and the field, on the current stream, and the result has the stream semantics of every other form
            out = self._flush_project(A_d)
            if not to_host:
                return out if wait else PendingField(out)
            return eng.to_host(out, result=True).T
        # the basis, centre and scale this object holds NOW: what the launch works on, whenever it is enqueued
        state = self._block()
        if defer:
            # defer_reconstruct: record the launch instead (the captured tensors stay alive with it)
            n_loc, n_p = state.Ur.shape[0], A_d.shape[0]
            total = int(self._shard_layout(n_loc)[:, 1].sum()) if self._dist() else n_loc
            pf = self._deferred = PendingField(None, launch=lambda: self._reconstruct_now(A_d, state, False, False),
                                               shape=(n_p, total), needs_cus=False)
            return pf
        return self._reconstruct_now(A_d, state, to_host, wait)

    def _defers(self):
        import os
        env = os.environ.get('SPR_DEFER_RECONSTRUCT')
        return (self.defer_reconstruct or env == '1') and env != '0'

    def _reconstruct_now(self, A_d, state, to_host, wait, path=None):
        """Enqueue the reconstruct kernel (and, sharded, the exchange of the field) on ``state``, the FittedBlock the
        caller took.  ``path``: 'p2p' / 'rccl' for this call only (the first-exchange trial), None: the object's choice."""
        eng = self._engine()
        n_loc = state.Ur.shape[0]
        n_p = A_d.shape[0]
        world = self._world()
        if not self._dist():
            if to_host and hasattr(eng, 'reconstruct_to_host'):
                # the reference's contract (:371-375): a host ndarray.  Big fields go out in row chunks whose copies run
                # under the next chunk's kernel, into page-locked memory (engine.reconstruct_to_host)
                host = eng.reconstruct_to_host(*state, A_d)
                if host is not None:
                    return host.T
            out = eng.reconstruct(*state, A_d)
        else:
            import torch.distributed as dist
            lay = self._shard_layout(n_loc)
            if (path or self._gather_select(n_p, lay)) == 'p2p':
                return self._reconstruct_p2p(A_d, state, lay, to_host, wait)
            if np.any(lay[:, 1] != n_loc):
                return self._gather_unequal(A_d, state, lay, to_host, wait)
            loc = eng.reconstruct(*state, A_d)
            # ONE all-gather for all n_p columns: rank q's (n_p, n_loc) block lands at stage[q]; for one column that is
            # the field itself, for several the columns are put side by side afterwards -- on the way to the host when
            # the caller wants a host array (block copies, no pass over the field on the device), by
            # spr_field_unstage_f64 when the field stays in HBM
            stage = eng.empty((world, n_p, n_loc))
            close = self._comm_bracket('gather')              # issue -> join, when the join happens inside this call
            import time
            self.last_comm_ = ('field all_gather (rccl)', (world, n_p, n_loc), time.time())
            nc = self._native_comm()
            if nc is not None:
                # the library's own communicator: the all-gather on a side stream behind the reconstruct kernel, joined by an event
                t = eng.torch
                side = self.__dict__.get('_comm_stream')
                if side is None:
                    side = self._comm_stream = t.cuda.Stream(eng.device)
                ev0 = t.cuda.Event()
                ev0.record(t.cuda.current_stream(eng.device))
                side.wait_event(ev0)
                with t.cuda.stream(side):
                    eng.comm_allgather(nc, loc, stage)
                    ev1 = t.cuda.Event()
                    ev1.record(side)
                loc.record_stream(side)
                stage.record_stream(side)

                class _Joined:
                    @staticmethod
                    def wait():
                        t.cuda.current_stream(eng.device).wait_event(ev1)
                work = _Joined()
            else:
                work = dist.all_gather_into_tensor(stage.view(-1), loc.contiguous().view(-1), group=self._shard.group,
                                                   async_op=True)
            if n_p == 1:
                out = stage.view(1, world * n_loc)
                if not to_host and not wait:
                    pf = PendingField(out, [work], keep=(loc, stage),
                                      on_wait=lambda: self._comm_bracket('gather_exposed'))
                    self._pending_field = pf                  # fit() leaves its host gap free while this is in flight
                    return pf
                work.wait()
                close()
            else:
                work.wait()
                close()
                if to_host and hasattr(eng, 'stage_to_host'):
                    host = eng.stage_to_host(stage)
                    if host is not None:
                        return host.T
                out = eng.field_unstage(stage)
                if not to_host and not wait:
                    return PendingField(out)
        if not to_host:
            return out if wait else PendingField(out)
        return eng.to_host(out, result=True).T                             # (n, n_p), Fortran-ordered view

    # ------------------------------------------------------------------ held-out snapshots (csrc/validate.hip)
    def _held_out(self, X, what):
        """X_new / X_true -> this rank's rows as a 2-D device matrix, stored as given (float64 or float32): an ndarray of
        shape (n, k) or (n,) is uploaded, a device tensor or a DeviceMatrix is used in place."""
        eng = self._engine()
        t = eng.torch
        n_loc = self.X.shape[0]
        if isinstance(X, DeviceMatrix):
            X = X.tensor
        dev = hasattr(X, 'is_cuda')
        if not dev:
            X = np.asarray(X)
        if X.ndim == 1:
            X = X[:, None]
        if X.ndim != 2:
            raise ValueError(f'{what} must have shape (n, k) or (n,), got {tuple(X.shape)}')
        if X.shape[0] != n_loc:
            raise ValueError(f'{what} has {X.shape[0]} rows, X has {n_loc}.')
        if dev:
            if X.dtype not in (t.float64, t.float32):
                raise TypeError(f'{what} must be float64 or float32, got {X.dtype}')
            return X if X.stride(1) == 1 or X.shape[1] == 1 else X.contiguous()
        f32 = X.dtype == np.float32
        return eng.to_device(X if f32 else np.asarray(X, dtype=np.float64), dtype=t.float32 if f32 else None)

    def transform(self, X_new):
        """Project held-out snapshots onto the basis on the device:  Ur^T ((X_new - X_cnt) / X_scl)  -- what users of the
        reference write on the host after fit() (docs/sparse_sensing_doc.ipynb), and the A_new its GPR.update(P_new, A_new)
        takes (gpr.py:603).  -> host ndarray (k, r), float64: the orientation of ``Ar`` and of what ``reconstruct`` takes.

        ``X_new``: ndarray of shape (n, k) or (n,), float64 or float32 (uploaded as stored), or a device tensor /
        DeviceMatrix (used in place); n = the rows of ``X`` (sharded: this rank's row block; the partial products are summed
        with one all-reduce).  One streaming pass over the basis and X_new; neither is copied to the host.

        It is Ur^T x0 for whatever basis the object holds -- fit(basis=...), an assigned ``Ur``, an f32-stored basis.  These
        are the least-squares coefficients of x0 in the basis only when Ur is orthonormal (the basis fit() computes)."""
        self._flush_deferred()
        eng = self._engine()
        blk = self._block(('encode',), 'validate.hip')
        Xd = self._held_out(X_new, 'X_new')
        if Xd.shape[1] == 0:
            return np.zeros((0, blk.Ur.shape[1]))
        return np.array(eng.to_host(self._all_reduce(eng.encode(*blk, Xd))), dtype=np.float64)

    def partial_fit(self, X_new, *, select_modes=None, n_modes=None, tol=1e-7):
        """Add the snapshots ``X_new`` to the fit without the snapshots it was computed from: the block incremental SVD
        (Brand 2002 / 2006; the rank-k update behind scikit-learn's IncrementalPCA).  The object keeps Ur, Sigma_r and the
        small Ar; a batch of k <= 64 columns costs three streaming passes over the basis and the batch --
        C = X0_b^T Ur (spr_encode_*), the residual pass H = E^T E, C2 = E^T Ur, ss = sum X0_b^2 with E = X0_b - Ur C^T formed
        on chip (spr_subspace_residual_*), and Ur <- Ur A + X0_b B into the spare basis buffer (spr_basis_update_*) -- and
        an SVD of size (r + k) on the host in between (_update.py).  ``rom.X`` is never read.

        ``X_new`` as ``transform`` takes it: ndarray (n, k) or (n,), float64 / float32 (uploaded as stored), a device
        tensor or a DeviceMatrix.  More than 64 columns are processed as consecutive 64-column slices, each a full update;
        no column: nothing happens.  X_cnt and X_scl stay those of the initial fit(): the batch is centred and scaled with
        them, as ``transform`` does.

        Rank after the update, with q = the directions of the batch whose residual exceeds ``tol`` * max(S[0], the largest
        residual): ``select_modes=None`` keeps r (fixed-rank streaming, constant memory); ``'number'``: min(n_modes, r + q);
        ``'variance'``: the smallest rank whose exp_variance_ reaches n_modes percent of all the energy seen, at most r + q.
        At most 128 modes.  A rank below r + q truncates: the result is then the usual truncated incremental SVD, close to
        the SVD of all snapshots but NOT equal to it (rank-200 data kept at 32 modes: reconstruction error 0.2741 against
        the optimal 0.2719, tests/test_partial_fit_host.py); what was cut is reported as ``dropped``.

        The energy of all snapshots seen starts as sum(Sigma_r^2) * 100 / exp_variance_[r - 1] of the fit and grows by ss.

        Updates Ur, Ar ((m_seen, r): a row per snapshot seen), Vr, Sigma_r, S_ (= Sigma_r), r, exp_variance_ (r,), n_seen_,
        and appends one dict per slice to ``partial_fit_info_``: ``q``, ``dropped`` (energy below tol plus energy cut by
        the rank), ``residual`` = sqrt(trace H' / ss) (the part of the batch outside the basis), ``orth_defect`` =
        |C2|_F / sqrt(trace H) (how far the held basis has drifted from orthonormal).  nrm0, Theta, C, cnt and the CPOD
        centre are dropped as fit() drops them.  ``X``, ``X0`` and scale_data still describe the initial block; a later
        fit() starts over from ``X``.

        Raises before anything is modified: ValueError (values that are not finite, seen in ss / H -- nothing n-sized is
        downloaded; a wrong row count), NotImplementedError (a rank above 128; a basis fit() did not compute in float64 --
        fit(basis=...), an assigned Ur, an f32 basis; a sharded object), AttributeError before fit() as ``transform``."""
        from . import _update
        self._flush_deferred()
        eng = self._engine()
        blk = self._block(('encode', 'subspace_residual', 'basis_update'), 'update.hip')
        if self._shard is not None:
            raise NotImplementedError('partial_fit is not built for sharded objects.')
        why = self.__dict__.get('_basis_foreign', 'no fit() of this object computed the basis')
        if why is not None:
            raise NotImplementedError('partial_fit updates the orthonormal float64 basis fit() computed together with Ar: '
                                      f'{why}.')
        Xd = self._held_out(X_new, 'X_new')
        if blk.Ur.shape[1] > _update.MAX_RANK:
            raise NotImplementedError(f'partial_fit is built for at most {_update.MAX_RANK} modes, the basis has '
                                      f'{blk.Ur.shape[1]}.')
        if select_modes not in (None, 'number', 'variance'):
            raise ValueError('The select_mode value is wrong.')
        for j0 in range(0, Xd.shape[1], _update.MAX_BATCH):
            self._partial_fit_slice(eng, Xd[:, j0:j0 + _update.MAX_BATCH], select_modes, n_modes, tol)

    def _partial_fit_slice(self, eng, Xb, select_modes, n_modes, tol):
        """One update of at most 64 columns (a column view of the caller's matrix); raises before any state changes"""
        from . import _update
        blk = self._block()
        Ur_d = blk.Ur
        n, r = Ur_d.shape
        S = np.asarray(self.Sigma_r, dtype=np.float64)
        Ar = np.asarray(self.Ar, dtype=np.float64)
        E_tot = self.__dict__.get('_pf_E_tot')
        if E_tot is None:
            E_tot = _update.initial_energy(S, self.exp_variance_)
        C_d = eng.encode(*blk, Xb)
        H_d, C2_d, ss_d = eng.subspace_residual(*blk, Xb, C_d)
        H, C2, ss = eng.to_host_views(H_d, C2_d, ss_d)
        C = np.array(eng.to_host(C_d), dtype=np.float64)
        up = _update.svd_update(S, Ar, C, H, C2, ss, E_tot, tol=tol, select_modes=select_modes, n_modes=n_modes)
        r2 = up['S'].shape[0]
        ld2 = r2 + (r2 & 1)                                  # the row stride project() gives a basis of r2 columns
        spare = self.__dict__.pop('_ur_spare', None)
        if not (spare is not None and tuple(spare.shape) == (n, r2) and spare.stride(0) == ld2 and spare.stride(1) == 1
                and spare.dtype == Ur_d.dtype and spare.data_ptr() != Ur_d.data_ptr()):
            spare = eng.empty((n, ld2))[:, :r2]
        new = eng.basis_update(*blk, Xb, eng.to_device(up['A']), eng.to_device(up['B']), out=spare)
        # ---- nothing above changed the object; from here on it holds the updated fit ----
        for k in ('C', 'Theta', '_cpod_Ar0'):
            self.__dict__.pop(k, None)
        for k in ('cnt', 'Theta', 'nrm0'):
            self._d.pop(k, None)
        self._host.pop('Ur', None)
        self._d['Ur'] = new
        self._ur_spare = Ur_d                                 # the old basis is the next update's target
        self.Ar = up['Ar']
        self.r = r2
        self.Sigma_r = up['S']
        self.S_ = up['S'].copy()
        with np.errstate(divide='ignore', invalid='ignore'):
            self.Vr = up['Ar'] / up['S']
        self.exp_variance_ = up['exp_variance']
        self._pf_E_tot = up['E_tot']
        self.n_seen_ = Ar.shape[0] + Xb.shape[1]
        self.__dict__.setdefault('partial_fit_info_', []).append(
            dict(q=up['q'], dropped=up['dropped'], residual=up['residual'], orth_defect=up['orth_defect']))

    def reconstruction_error(self, X_true, Ar=None):
        """Error per feature of ``reconstruct(Ar)`` against the true field ``X_true`` (physical units), formed on the device:
        the reconstruct pass with a comparison in place of the store -- the field is neither written nor copied to the host.
        ``X_true`` as ``transform`` takes X_new, (n, k) or (n,); ``Ar`` of shape (k, r) or (r,).  ``Ar=None`` uses
        ``transform(X_true)``: the truncation error of the basis, the best any predict() can reach.

        -> dict of host arrays per vector and feature, shape (k, F):  ``sse`` = sum d^2,  ``ss_true`` = sum X_true^2,
        ``max_abs`` = max |d|,  ``max_row`` (int64) = the lowest global row attaining it,  ``rel_l2`` = sqrt(sse / ss_true),
        ``rmse`` = sqrt(sse / n_points);  and ``rel_l2_total`` (k,) over all features.

        Sharded objects: every rank sweeps its block, ONE all-gather of the ranks' (k, F, 4) records; the sums are added in
        rank order and the maxima merged (lowest global row on a tie) identically on every rank."""
        self._flush_deferred()
        eng = self._engine()
        blk = self._block(('field_error',) if Ar is not None else ('field_error', 'encode'), 'validate.hip')
        Xd = self._held_out(X_true, 'X_true')
        k, r = Xd.shape[1], blk.Ur.shape[1]
        if Ar is not None:
            A_d = self._coefficients(eng, Ar, lambda A: None if tuple(A.shape) == (k, r) else
                                     f'Ar has shape {tuple(A.shape)}; X_true has {k} columns and the basis {r} modes.')
        if k == 0:
            raise ValueError('X_true has no columns.')
        if Ar is None:
            A_d = self._all_reduce(eng.encode(*blk, Xd))        # (k, r), summed over the ranks
        rec_d = eng.field_error(*blk, A_d, Xd)
        rec = np.asarray(eng.to_host(self._all_gather(rec_d)), dtype=np.float64)       # (world, k, F, 4)
        sse, ss_true = rec[..., 0].sum(axis=0), rec[..., 1].sum(axis=0)
        held = rec[..., 3] >= 0                                                         # ranks with rows of the feature
        v = np.where(held, rec[..., 2], -np.inf)
        max_abs = v.max(axis=0)
        rows = np.where(held & (v == max_abs), rec[..., 3], np.inf).min(axis=0)
        max_row = np.where(np.isfinite(rows), rows, -1).astype(np.int64)
        with np.errstate(divide='ignore', invalid='ignore'):
            rel_l2 = np.sqrt(sse / ss_true)
            rel_tot = np.sqrt(sse.sum(axis=1) / ss_true.sum(axis=1))
        return dict(sse=sse, ss_true=ss_true, max_abs=np.where(np.isfinite(max_abs), max_abs, 0.0), max_row=max_row,
                    rel_l2=rel_l2, rmse=np.sqrt(sse / self.n_points), rel_l2_total=rel_tot)

    # ------------------------------------------------------------------ gappy POD (csrc/gappy.hip)
    def _gappy_mask(self, eng, mask, Xd):
        """mask argument -> uint8 device tensor of shape (n,) or (n, k), non-zero = observed; None: where X_obs is finite"""
        t = eng.torch
        n_loc, k = Xd.shape
        if mask is None:
            return t.isfinite(Xd).view(t.uint8)               # formed on the device, per column; never downloaded
        dev = hasattr(mask, 'is_cuda')
        if not dev:
            mask = np.asarray(mask)
        if mask.dtype not in ((t.bool, t.uint8) if dev else (np.bool_, np.uint8)):
            raise TypeError(f'mask must be bool or uint8, got {mask.dtype}')
        if mask.ndim not in (1, 2) or (mask.ndim == 2 and mask.shape[1] != k):
            raise ValueError(f'mask must have shape (n,) or (n, {k}), got {tuple(mask.shape)}')
        if mask.shape[0] != n_loc:
            raise ValueError(f'mask has {mask.shape[0]} rows, X has {n_loc}.')
        if not dev:
            mask = eng.to_device(mask.view(np.uint8), dtype=t.uint8)
        elif mask.dtype == t.bool:
            mask = mask.view(t.uint8)
        return mask if mask.is_contiguous() else mask.contiguous()

    def _gappy_groups(self, eng, M):
        """Columns of the (n, k) device mask with identical masks -> group id per column (host, numbered by first column).
        Identity is decided by an exact comparison on the device; the column counts only pre-sort (columns with different
        counts cannot be equal).  Only k-sized vectors come to the host.  Sharded: two columns belong together when they
        do on EVERY rank -- one all-gather of the ranks' k labels."""
        t = eng.torch
        k = M.shape[1]
        Mb = M != 0                                           # any non-zero byte means observed
        cnt = Mb.sum(dim=0, dtype=t.int64).cpu().numpy()
        label = np.full(k, -1, dtype=np.int64)
        for c in np.unique(cnt):
            cols = np.flatnonzero(cnt == c)
            while len(cols):
                rep = int(cols[0])
                if len(cols) == 1:
                    same = np.array([True])
                else:
                    same = (Mb[:, cols.tolist()] == Mb[:, rep:rep + 1]).all(dim=0).cpu().numpy()
                label[cols[same]] = rep
                cols = cols[~same]
        if self._dist():
            lab = np.asarray(eng.to_host(self._all_gather(eng.to_device(label.astype(np.float64)))))     # (world, k)
            _, first, inv = np.unique(np.rint(lab).astype(np.int64), axis=1, return_index=True, return_inverse=True)
            label = first[np.ravel(inv)]
        _, group = np.unique(label, return_inverse=True)      # labels are first columns: increasing label = order of appearance
        return np.ravel(group).astype(np.int64)

    def gappy_transform(self, X_obs, mask=None, *, rcond=1e-12, return_cov=False):
        """Gappy POD: least-squares coefficients of partially observed snapshots in the basis, formed on the device,
        a_j = (Ur^T M_j Ur)^+ Ur^T M_j x0_j  with  x0 = (X_obs - X_cnt) / X_scl  and M_j the 0/1 row mask of column j -- what
        np.linalg.lstsq(Ur[m_j], x0[m_j, j]) gives on the host.  -> host ndarray (k, r), float64, the orientation of ``Ar``:
        ``reconstruct`` repairs the field from it, ``reconstruction_error(X_true, Ar=...)`` scores the repair.

        ``X_obs``: as ``transform`` takes X_new -- (n, k) or (n,), float64 / float32 stored as given, an ndarray, a device
        tensor or a DeviceMatrix; sharded: this rank's row block.  Unobserved entries are never used: they may hold NaN.
        ``mask``: bool / uint8 ndarray or device tensor, non-zero = observed; shape (n,): one mask for all columns, (n, k):
        one per column; None: observed where X_obs is finite, per column (formed on the device, never downloaded).

        One streaming pass over the basis and the columns per GROUP of columns with identical masks (csrc/gappy.hip: the
        masked Gram matrix H = Ur^T M Ur and B = X0^T M Ur on the f64 MFMA; 64-row panels without an observed row are
        skipped before they are read); identity of masks is established exactly, on the device.  Distinct masks cost one
        pass each.  The r x r solve runs on the host in f64: H is symmetrised, eigh, eigenvalues lambda > rcond lambda_max
        are kept and a = V diag(1 / lambda) V^T b -- the minimum-norm least-squares solution, np.linalg.pinv(M Ur) @ x0 with
        its cut placed on sigma^2 = lambda.  The default rcond = 1e-12 is on the eigenvalues of the Gram matrix, i.e.
        sigma_min / sigma_max = 1e-6: beyond it the normal equations have lost the solution in f64 anyway.  A column
        without an observed row gives a = 0 (rank 0).

        ``return_cov=True``: also (k, r, r), H_j^+ per column -- the covariance of the coefficients for unit i.i.d. noise on
        the scaled observations; ``reconstruct_std(cov=sigma**2 * that)`` is the field uncertainty of the repair.  Columns
        of one group share one matrix (a single group: a read-only broadcast view).

        ``gappy_info_``: dict of per-column arrays ``n_observed`` (int64, global), ``rank``, ``cond`` =
        sqrt(lambda_max / lambda_min kept) (inf at rank 0), ``group``, and the scalars ``groups`` and ``passes`` (reads of
        the basis).  It is the least-squares fit in whatever basis the object holds (fit(basis=...), an assigned ``Ur``, f32
        storage); orthonormality is not assumed.  r <= 128.  Sharded objects: ONE all-reduce of the [H | B | n_observed]
        buffer per group (and one all-gather of k labels when there are per-column masks); every rank solves the same bits."""
        self._flush_deferred()
        eng = self._engine()
        blk = self._block(('gappy_normal',), 'gappy.hip')
        r = blk.Ur.shape[1]
        if r > SPR_MAX_R:
            raise ValueError(f'gappy_transform takes bases of up to {SPR_MAX_R} modes, this one has {r}; keep fewer modes.')
        rcond = float(rcond)
        if not 0.0 <= rcond < 1.0:
            raise ValueError(f'rcond must lie in [0, 1), got {rcond}')
        Xd = self._held_out(X_obs, 'X_obs')
        k = Xd.shape[1]
        M = self._gappy_mask(eng, mask, Xd)
        if k == 0:
            self.gappy_info_ = dict(n_observed=np.zeros(0, dtype=np.int64), rank=np.zeros(0, dtype=np.int64),
                                    cond=np.zeros(0), group=np.zeros(0, dtype=np.int64), groups=0, passes=0)
            return (np.zeros((0, r)), np.zeros((0, r, r))) if return_cov else np.zeros((0, r))
        group = np.zeros(k, dtype=np.int64) if (M.dim() == 1 or k == 1) else self._gappy_groups(eng, M)
        n_groups = int(group.max()) + 1
        A = np.zeros((k, r))
        covs = [None] * n_groups
        n_obs, rank, cond = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.int64), np.full(k, np.inf)
        passes = 0
        for g in range(n_groups):
            cols = np.flatnonzero(group == g)
            j0, kg = int(cols[0]), len(cols)
            if kg == k:
                Xg = Xd
            elif cols[-1] - j0 + 1 == kg:
                Xg = Xd[:, j0:j0 + kg]                        # neighbours: a view, the row stride stays
            else:
                Xg = Xd[:, cols.tolist()]                     # a device-side gather of the group's columns
            mg = M if M.dim() == 1 else M[:, j0]              # one column of the row-major mask: element stride k
            H_d, B_d, nobs_d = eng.gappy_normal(*blk, Xg, mg)
            flat = H_d._base
            if flat is None or flat.numel() != r * r + kg * r + 1:
                raise RuntimeError('gappy_normal must return views of one [H | B | nobs] buffer')
            host = np.array(eng.to_host(self._all_reduce(flat)), dtype=np.float64)
            H, B, nobs = host[:r * r].reshape(r, r), host[r * r:r * r + kg * r].reshape(kg, r), host[-1]
            passes += -(-kg // 64)
            n_obs[cols] = int(round(nobs))
            lam, V = np.linalg.eigh(0.5 * (H + H.T))          # ascending
            keep = lam > rcond * lam[-1] if lam[-1] > 0 else np.zeros(r, dtype=bool)
            Vk, lk = V[:, keep], lam[keep]
            A[cols] = ((B @ Vk) / lk) @ Vk.T
            rank[cols] = int(keep.sum())
            if keep.any():
                cond[cols] = np.sqrt(lam[-1] / lk.min())
            if return_cov:
                P = (Vk / lk) @ Vk.T
                covs[g] = 0.5 * (P + P.T)                     # exactly symmetric
        self.gappy_info_ = dict(n_observed=n_obs, rank=rank, cond=cond, group=group, groups=n_groups, passes=passes)
        if not return_cov:
            return A
        if n_groups == 1:
            return A, np.broadcast_to(covs[0], (k, r, r))
        cov = np.empty((k, r, r))
        for g in range(n_groups):
            cov[group == g] = covs[g]
        return A, cov

    # ------------------------------------------------------------------ POD from incomplete snapshots (csrc/gappy_fill.hip)
    _GAPPY_COUNT_ROWS = 1 << 22    # rows per block of fit_gappy's column count

    def fit_gappy(self, mask=None, *, max_iter=100, tol=1e-6, scale_type='std', axis_cnt=1, select_modes='variance',
                  n_modes=99):
        """fit() for a snapshot matrix with holes: the iteration of Everson & Sirovich (1995; DINEOF in geophysics) --
        fill the holes, POD, re-fill them with the rank-r reconstruction, until the holes stop moving -- with every pass
        over the matrix on the device (csrc/gappy_fill.hip).

        1. every hole gets the mean of the observed entries of its row;  2. ``fit(scale_type, axis_cnt, select_modes,
        n_modes)``;  3. every hole (i, j) gets ``X_scl[f(i)] (Ur[i] . Ar[j]) + X_cnt[i]``, what ``reconstruct(Ar)`` puts
        there, and the pass returns S_d = sum over holes (new - old)^2 and S_n = sum over holes new^2;  4. ``fit(...)``
        again;  5. stop when delta = sqrt(S_d / S_n) <= ``tol`` or after ``max_iter`` fill passes, else back to 3.  The
        method always ends with a fit() of the matrix the object now holds, so every fitted attribute is exactly what
        fit() leaves for the filled matrix and everything downstream (placement, train, predict, transform, CPOD, ...)
        works unchanged.  Without convergence after ``max_iter`` passes a RuntimeWarning is issued and the object is left
        fitted.  A matrix without holes takes one plain fit() and no fill pass.

        ``mask``: (n, m) bool / uint8 ndarray or device tensor, non-zero = observed (sharded: this rank's rows); None:
        observed where X is finite, formed on the device and never downloaded.  It stays in HBM for the whole call as one
        byte per entry (23 GB beside the 184 GB of X and the 46 GB of basis at BASELINE config 3; bit-packed masks are not
        built).  Before anything is modified: every row and every column (over all ranks) must have an observed entry and
        every observed entry must be finite, else ValueError naming the lowest global row / the column; so does a number
        of modes beyond 128 where it is known in advance (select_modes='number', or 100 % variance).  With
        select_modes='variance' below 100 % the number of modes is only known after a fit(): if that keeps more than 128,
        ValueError is raised with the holes already holding their row means (or an earlier fill).

        IN PLACE: a caller's DeviceMatrix (its device tensor) is filled where it lies -- a copy of 184 GB is not an option;
        its observed entries keep their bytes.  A caller's host ndarray is not touched: the object's device copy is
        filled and ``self.X`` becomes a DeviceMatrix over it (storage dtype and ``basis='f32'`` kept), so ``rom.X``, a pickle
        and ``X0`` describe the matrix that was fitted.

        ``gappy_fit_info_``: dict with ``iterations`` (fill passes), ``converged``, ``delta`` (one per fill pass), ``holes``
        (global count), ``r`` (one per fit(): select_modes='variance' may change it between iterations) and ``passes``
        (fit() calls).  Sharded objects: the fills are row-local; one all-reduce of the m column counts, one all-gather of
        the row-fill record and one all-reduce of (S_d, S_n) per iteration -- every rank sees the same delta and stops at the
        same iteration (a rank whose own block is valid has row-mean values in its holes when another rank's block is
        refused).  No atomics: two runs agree bit for bit."""
        import warnings
        self._flush_deferred()
        eng = self._engine_with(('gappy_rowfill', 'gappy_fill'), 'gappy_fill.hip')
        if type(max_iter) is not int or max_iter < 1:
            raise ValueError(f'max_iter must be a positive integer, got {max_iter!r}')
        tol = float(tol)
        if not tol >= 0.0:
            raise ValueError(f'tol must be non-negative, got {tol}')
        self._check_scaling(scale_type, axis_cnt)
        if select_modes not in ('variance', 'number'):
            raise ValueError('The select_mode value is wrong.')
        fit_args = (scale_type, axis_cnt, select_modes, n_modes)
        t = eng.torch
        Xd = self._Xd()
        m = Xd.shape[1]
        if select_modes == 'number' or n_modes == 100:
            r0 = self._select_rank(None, m, select_modes, n_modes)
            if r0 > SPR_MAX_R:
                raise ValueError(f'fit_gappy fills the holes from bases of up to {SPR_MAX_R} modes, {r0} were asked for; keep '
                                 'fewer modes.')
        M = self._gappy_mask(eng, mask, Xd)
        if M.dim() != 2:
            raise ValueError(f'mask must have shape (n, {m}), got {tuple(M.shape)}')
        # every column observed somewhere: one all-reduce of m counts (exact in f64)
        colc = eng.zeros((m,))
        for i0 in range(0, M.shape[0], self._GAPPY_COUNT_ROWS):   # row blocks: the comparison's temporary stays small
            colc += t.count_nonzero(M[i0:i0 + self._GAPPY_COUNT_ROWS], dim=0)
        cols = np.asarray(eng.to_host(self._all_reduce(colc)))
        if np.any(cols == 0):
            raise ValueError(f'column {int(np.flatnonzero(cols == 0)[0])} of X has no observed entry.')
        # row means into the holes -- the kernel validates first and writes nothing into a block with a bad row
        rec = np.asarray(eng.to_host(self._all_gather(eng.gappy_rowfill(Xd, self._row0, M))), dtype=np.float64)   # (world, 8)
        for cnt, row, what in ((1, 2, 'has no observed entry'), (3, 4, 'holds an observed entry that is not finite')):
            if rec[:, cnt].sum() > 0:
                low = int(rec[rec[:, cnt] > 0, row].min())
                raise ValueError(f'row {low} of X {what}.')
        holes = int(rec[:, 0].sum())
        info = dict(iterations=0, converged=True, delta=[], holes=holes, r=[], passes=0)
        self.gappy_fit_info_ = info
        if holes == 0:
            self.fit(*fit_args)
            info['r'].append(int(self.r))
            info['passes'] = 1
            return
        if not isinstance(self.X, DeviceMatrix):
            self.X = DeviceMatrix(Xd, basis='f32' if self._basis_dtype() == t.float32 else None)
        info['converged'] = False
        self.fit(*fit_args)
        info['r'].append(int(self.r))
        info['passes'] = 1
        while info['iterations'] < max_iter:
            if self.r > SPR_MAX_R:
                raise ValueError(f'fit_gappy fills the holes from bases of up to {SPR_MAX_R} modes, fit() kept {self.r}; keep '
                                 'fewer modes.  The holes of X already hold their row means (or an earlier fill) and the '
                                 'object is fitted to that matrix.')
            pend = self.__dict__.get('_pending')
            A_d = pend['Ar'] if pend is not None else eng.to_device(np.ascontiguousarray(self.Ar, dtype=np.float64))
            out = eng.gappy_fill(*self._block(), A_d, Xd, M)        # (the block of the fit() just done)
            s_d, s_n = np.asarray(eng.to_host(self._all_reduce(out)), dtype=np.float64)[:2]
            with np.errstate(divide='ignore', invalid='ignore'):
                delta = float(np.sqrt(s_d / s_n)) if s_n > 0 or s_d > 0 else 0.0
            info['iterations'] += 1
            info['delta'].append(delta)
            self.fit(*fit_args)
            info['r'].append(int(self.r))
            info['passes'] += 1
            if delta <= tol:
                info['converged'] = True
                break
        if not info['converged']:
            warnings.warn(f'fit_gappy did not converge in {max_iter} fill passes: delta = {info["delta"][-1]:.3e} > tol = '
                          f'{tol:.3e}; the object is fitted to the matrix as it is now.', RuntimeWarning, stacklevel=2)

    # ------------------------------------------------------------------ field uncertainty (csrc/field_std.hip)
    @staticmethod
    def _cov_factors(cov):
        """(k, r, r) covariances -> factors L (k, r, q) with cov_j = L_j L_j^T, q = the largest retained rank of the batch
        (zero columns behind a lower rank); None when every matrix is zero."""
        sym = 0.5 * (cov + cov.transpose(0, 2, 1))
        if not np.all(np.isfinite(sym)):
            raise ValueError('cov has entries that are not finite')
        lam, V = np.linalg.eigh(sym)                          # ascending, batched
        lmax = lam[:, -1]
        if np.any(lam[:, 0] < -1e-12 * lmax):
            raise ValueError('cov is not positive semi-definite')
        keep = lam > 1e-15 * lmax[:, None]
        q = int(keep.sum(axis=1).max())
        if q == 0:
            return None
        k, r = lam.shape
        L = np.zeros((k, r, q))
        for j in range(k):
            sel = np.flatnonzero(keep[j])[::-1]               # largest eigenvalue first
            L[j, :, :len(sel)] = V[j][:, sel] * np.sqrt(lam[j, sel])
        return L

    def reconstruct_std(self, sigma=None, *, cov=None, factor=None, to_host=True):
        """Per-cell standard deviation of ``reconstruct(Ar)`` when the coefficients carry a Gaussian uncertainty, formed on
        the device: linear propagation through  x = X_scl (Ur a) + X_cnt,  so  std_i = X_scl sqrt((Ur Sigma Ur^T)_ii).
        Neither the basis nor anything r-by-n goes to the host.  Exactly one of

        ``sigma``   (k, r) or (r,): independent per-coefficient standard deviations -- the orientation of predict()'s
                    ``Ar_sigma`` and of the reference's ``GPR.predict`` ``Sigmap``;  X_scl sqrt((Ur**2) @ sigma**2).
        ``cov``     (k, r, r) or (r, r): full coefficient covariances, e.g. ``SPR.coefficient_covariance(y)``.  Symmetrised
                    and factored on the host (eigh): an eigenvalue below -1e-12 lambda_max raises
                    ValueError('cov is not positive semi-definite'), eigenvalues up to 1e-15 lambda_max are dropped.
        ``factor``  (k, r, q) or (r, q), 1 <= q <= r: factors L with covariance L L^T;  X_scl |L^T u_i|_2.  ``cov`` and
                    ``factor`` take bases of up to 128 modes.

        -> host ndarray (n, k), float64, the orientation ``reconstruct`` returns; ``to_host=False``: the device tensor
        (k, n).  It holds for whatever basis the object has (fit(basis=...), an assigned ``Ur``, an f32-stored basis): the
        formula needs no orthonormality.  Sharded objects: every rank sweeps its block, ONE all-gather of the blocks
        (padded to the largest), cut to the ranks' rows on the host; ``to_host=False`` returns THIS RANK's block (k, n_loc)
        only.  There is no ``sampling=``: the reference's sampled un-scaling is not a variance-preserving map."""
        self._flush_deferred()
        if sum(x is not None for x in (sigma, cov, factor)) != 1:
            raise ValueError('reconstruct_std takes exactly one of sigma, cov and factor.')
        eng = self._engine()
        blk = self._block(('field_std',), 'field_std.hip')
        std_args = (*blk[:4], blk.scale)                      # field_std takes no centre
        n_loc, r = blk.Ur.shape
        S = L = None
        if sigma is not None:
            S = self._coefficients(eng, sigma, lambda A: None if A.ndim == 2 and A.shape[1] == r else
                                   f'sigma must have shape (k, {r}) or ({r},), got {tuple(np.shape(sigma))}.')
            k = S.shape[0]
        else:
            name, M = ('cov', cov) if cov is not None else ('factor', factor)
            dev = hasattr(M, 'is_cuda') and cov is None
            M = M if dev else np.asarray(M, dtype=np.float64)
            if M.ndim == 2:
                M = M[None]
            ok = M.ndim == 3 and M.shape[1] == r and (M.shape[2] == r if cov is not None else 1 <= M.shape[2] <= r)
            if not ok:
                want = f'(k, {r}, {r}) or ({r}, {r})' if cov is not None else f'(k, {r}, q) or ({r}, q) with 1 <= q <= {r}'
                raise ValueError(f'{name} must have shape {want}, got {tuple(np.shape(cov if cov is not None else factor))}.')
            if r > SPR_MAX_R:
                raise ValueError(f'reconstruct_std({name}=...) takes bases of up to {SPR_MAX_R} modes, this one has {r}; '
                                 'sigma= takes any.')
            k = M.shape[0]
            L = M if (cov is None or k == 0) else self._cov_factors(M)
        dist_ = self._dist()
        n_out = self._n_global if (to_host or not dist_) else n_loc
        if k == 0:
            return np.zeros((n_out, 0)) if to_host else eng.empty((0, n_out))
        if S is None and L is None:                           # every covariance is zero: a zero map, nothing to launch
            return np.zeros((n_out, k)) if to_host else eng.zeros((k, n_out))
        if L is not None and not hasattr(L, 'is_cuda'):
            L = eng.to_device(L)
        if not dist_ or not to_host:
            out = eng.field_std(*std_args, S=S, L=L)
            return eng.to_host(out, result=True).T if to_host else out
        lay = self._shard_layout(n_loc)
        n_max = int(lay[:, 1].max())
        buf = eng.zeros((k, n_max)) if n_max > n_loc else eng.empty((k, n_max))
        eng.field_std(*std_args, S=S, L=L, out=buf[:, :n_loc])
        blocks = np.asarray(eng.to_host(self._all_gather(buf)))                         # (world, k, n_max)
        return np.concatenate([blocks[q, :, :int(lay[q, 1])] for q in range(len(lay))], axis=1).T


class SPR(GemPlacement, DesignPlacement, ROM):
    """Sparse Placement for Reconstruction (reference: SPR, sparse_sensing.py:513-901)."""

    placement_norms = None      # "auto": see ROM.placement_norms

    #: optimal_placement('qr') on one rank: between two passes over the whole basis, refresh only the rows whose norm can
    #: still win a step (pivot_loop / _pivot_loop_pooled).  Same sensors; False: one full sweep per batch of steps.
    placement_pools = True

    def __init__(self, X, n_features, xyz, shard=None, engine=None):
        super().__init__(X, n_features, xyz, shard=shard, engine=engine)

    def _check_rank_cap(self, what):
        """The placement and solve kernels are built for bases of up to SPR_MAX_R_WIDE columns (the reference takes any
        r <= m, :336, :739): say so BEFORE any device work, naming the cap."""
        if self.r > SPR_MAX_R_WIDE:
            raise ValueError(f'{what}: r = {self.r} retained modes exceed the {SPR_MAX_R_WIDE} the placement and solve '
                             'kernels are built for (fit and reconstruct take any r); keep fewer modes.')

    # ------------------------------------------------------------------ a6 optimal_placement
    def optimal_placement(self, calc_type='qr', n_sensors=10, mask=None, d_min=0., verbose=False):
        """Reference :700-756.  Returns the one-hot measurement matrix C of shape (s, n): the reference's dense ndarray
        while it is small (64 MiB), a OneHotRows above that (46 GB dense at BASELINE config 3) -- same behaviour for
        C[i, :], C @ x, np.argmax(C, axis=1), train(C).  The ordered global sensor rows are also in ``self.sensors_``."""
        self._flush_deferred()
        if calc_type == 'gem':
            return self._placement_gem(n_sensors, mask, d_min, verbose)
        if calc_type in ('dopt', 'aopt'):                     # 'qr', then greedy D / A-optimal additions (_design.py)
            return self._placement_design(calc_type, n_sensors, mask, d_min)
        if calc_type != 'qr':
            raise NotImplementedError('The sensor selection method has not been implemented yet')
        eng = self._engine()
        n = self._n_global
        Ur_d = self._fitted('Ur', 'Ur')
        self._check_rank_cap('optimal_placement')
        if mask is not None:
            mask = np.asarray(mask)
            _check_mask(mask, Ur_d.shape[0])
            eng.mask_rows(Ur_d, eng.to_device(mask.astype(np.uint8), dtype=eng.torch.uint8))   # :737-738
            self._host.pop('Ur', None)
            self._d.pop('nrm0', None)                         # rows were zeroed: the norms fit() left no longer hold
            self._basis_foreign = 'optimal_placement(mask=...) zeroed rows of the basis'   # (CPOD)
        s = self.r
        nrm0 = self._d.get('nrm0')                            # left by fit() under placement_norms, for this very basis
        self.placement_from_norms_ = nrm0 is not None and nrm0.shape[0] == Ur_d.shape[0]
        if self.placement_from_norms_:
            st = eng.qr_begin(Ur_d, self._row0, s, norms=nrm0)
        else:
            st = eng.qr_begin(Ur_d, self._row0, s)
        stats = {}
        sweeps = pivot_loop(eng, st, s, self._all_gather if self._dist() else None, pools=self.placement_pools,
                            stats=stats)
        self.pivot_sweeps_ = sweeps - int(self.placement_from_norms_)   # passes over the basis (the start read none)
        self.pivot_pool_sweeps_ = stats.get('pool_sweeps', 0)           # refreshes that visited the pool only
        self.pivot_log_ = stats.get('log', [])                          # batches and refreshes of the pooled driver, in order
        piv = eng.to_host(st['piv']).astype(np.int64)
        self.sensors_ = piv
        self.pivot_gap_ = eng.to_host(st['gap'])
        C = self._one_hot(piv, n)
        self._placed = (C, piv)
        return C

    @staticmethod
    def _one_hot(piv, n):
        """(s, n) one-hot matrix of the picks (:741-743): the reference's dense ndarray while it is small, a OneHotRows
        (same behaviour for the documented uses, s integers of storage) above _DENSE_C_LIMIT bytes."""
        C = OneHotRows(piv, n)
        return C.toarray() if len(piv) * n * 8 <= _DENSE_C_LIMIT else C

    # ------------------------------------------------------------------ a7 train
    def train(self, C, is_Theta=False, limits=None, method='OLS', solver='CLARABEL', cond=False, verbose=False):
        """Reference :758-820."""
        self._flush_deferred()
        n = self._n_global
        if (C.shape[1] != n) and not is_Theta:
            raise ValueError('The number of columns of C does not match the number'
                             ' of rows of X.')
        eng = self._engine()
        if method == 'COLS' and not hasattr(eng, 'bound_sweep'):
            raise NotImplementedError("method='COLS' needs the engine's bound sweep (csrc/bounds.hip); this engine has "
                                      'none (no CPU fallback).')
        if not is_Theta:
            placed = getattr(self, '_placed', None)
            known = None
            if placed is not None and placed[0] is C:
                piv = placed[1]
                known = (np.arange(len(piv) + 1), piv, np.ones(len(piv)))
            ip, ix, v = self._csr_device(C, known)
            Theta_d, cnt_d = eng.measure_csr(ip, ix, v, self._fitted('Ur', 'Ur'), self._row0,
                                             self._fitted('rowmean', 'X_cnt'))
            Theta_d = self._all_reduce(Theta_d)
            cnt_d = self._all_reduce(cnt_d)
            self.C = C
            self._d['cnt'] = cnt_d
            Theta = eng.to_host(Theta_d)
        else:
            Theta = np.asarray(C, dtype=np.float64)
            Theta_d = None
        if Theta.shape[1] != self.r:
            raise ValueError('The number of columns of Theta does not match the number'
                             ' of columns of Ur.')
        self._d['Theta'] = Theta_d if Theta_d is not None else eng.to_device(Theta)
        self.Theta = Theta
        self.limits = limits
        self.method = method
        self.solver = solver
        self.verbose = verbose
        if method == 'COLS':
            self._cols_cnt_minmax = self._feature_cnt_minmax()   # for the +-1000 clamps; once per train
        if cond == True:                                      # noqa: E712  (:813-820; s x r, host-sized)
            if Theta.shape[0] == Theta.shape[1]:
                S_theta = np.linalg.svd(Theta, compute_uv=False)
            else:
                S_theta = np.linalg.svd(np.linalg.pinv(Theta), compute_uv=False)
            self.k = S_theta[0] / S_theta[-1]

    # ------------------------------------------------------------------ a8 / a9
    _PINV_RCOND = 1e-15    # np.linalg.pinv's default in the reference's NumPy (:873, :877)

    @staticmethod
    def _download_solve(eng, Ar_d, As_d, y0_d, info_d):
        """-> (info, fetch): info on the host now; fetch() -> (Ar, Ar_sigma, y0) on the host.  With to_host_views the four
        outputs come down in ONE download (they share a buffer), else info now and the other three when asked for."""
        many = getattr(eng, 'to_host_views', None)
        if many is not None:
            info, *rest = many(info_d, Ar_d, As_d, y0_d)
            return info, lambda: tuple(rest)
        return eng.to_host(info_d), lambda: (eng.to_host(Ar_d), eng.to_host(As_d), eng.to_host(y0_d))

    def _solve(self, ys):
        """scale_vector + (weighted) least squares for a list of measurement vectors, on the device.
        Full-column-rank, well-conditioned systems take the MFMA normal-equations kernel; everything else the
        reference's pinv accepts -- fewer sensors than modes (every GEM placement), rank-deficient W Theta,
        cond^2 beyond what the refined normal equations resolve -- takes the QR + one-sided-Jacobi SVD kernel
        with the same rcond cut, which returns the minimum-norm solution exactly as np.linalg.pinv does."""
        eng = self._engine()
        if 'cnt' not in self._d:
            raise AttributeError("'SPR' object has no attribute 'C'")      # reference fails at self.C (:573)
        Theta_d, cnt_d = self._d['Theta'], self._d['cnt']
        self._check_rank_cap('predict')
        if cnt_d.shape[0] != Theta_d.shape[0]:
            # train(Theta, is_Theta=True) after train(C) with another sensor count: C.dot(X_cnt) (:573) no longer
            # matches the rows of y -- the reference fails with a broadcast error at :578
            raise ValueError(f'operands could not be broadcast together: y has {Theta_d.shape[0]} rows, '
                             f'C has {cnt_d.shape[0]}')
        Yh = np.stack([np.asarray(y, dtype=np.float64) for y in ys])
        fid = Yh[:, :, 2].astype('int')                                   # :576 indexes X_scl with it
        n_loc_rows = self._n_global
        bad = (fid * self.n_points >= n_loc_rows) | (fid * self.n_points < -n_loc_rows)
        if bad.any():
            k = int(fid.ravel()[np.argmax(bad.ravel())]) * self.n_points
            raise IndexError(f'index {k} is out of bounds for axis 0 with size {n_loc_rows}')
        if (fid < 0).any():                                               # numpy wraps negative indices (:576)
            Yh = Yh.copy()
            Yh[:, :, 2] = np.where(fid < 0, fid + self.n_features, fid)
        Y = eng.to_device(Yh)
        s, r = Theta_d.shape
        if s >= r and r <= getattr(eng, 'ols_max_r', r):      # the normal-equations kernel keeps its factor in LDS
            info, fetch = self._download_solve(eng, *eng.solve_ols(Theta_d, cnt_d, self._d['scale'], Y))
            if np.any(info[:, 0] == 2):
                # an uncertainty that is zero (or NaN) for SOME sensors of a vector: W = diag(1/0) (:872) and
                # np.linalg.pinv(W @ Theta) (:873) raises -- flagged by the kernel, no second solve
                raise np.linalg.LinAlgError('SVD did not converge')
            # the kernel's refinement step (corrected semi-normal equations) is as accurate as a QR solve while
            # cond(W Theta)^2 eps < 1; info[:, 1] estimates cond^2 from the Cholesky pivots
            if not (np.any(info[:, 0] != 0) or np.any(info[:, 1] > 1e13) or not np.all(np.isfinite(info[:, 1]))):
                self.solve_path_ = 'cholesky'
                return fetch()
        info, fetch = self._download_solve(eng, *eng.solve_pinv(Theta_d, cnt_d, self._d['scale'], Y, rcond=self._PINV_RCOND))
        if np.any(info[:, 0] < 0):
            raise np.linalg.LinAlgError('SVD did not converge')           # what np.linalg.pinv raises
        self.solve_path_ = 'pinv'
        self.solve_rank_ = info[:, 1].astype(int)
        return fetch()

    def scale_vector(self, y):
        """Reference :553-584.  Returns y0 (s,2); sets cnt_vector / scl_vector."""
        _, _, y0 = self._solve([y])
        self.cnt_vector = self._engine().to_host(self._d['cnt'])
        self.scl_vector = self._scl_f[np.asarray(y)[:, 2].astype('int')]
        return y0[0]

    def coefficient_covariance(self, y):
        """Covariance of the coefficients ``predict(y)`` returns, for independent sensor noise with the standard deviations
        in y[:, 1]:  P P^T  with  P = pinv(W Theta),  W = diag(1 / y0[:, 1]),  y0[:, 1] = y[:, 1] / scl  as predict scales it
        (the solve is  a = P W y0, and W y0 has unit covariance).  ``y`` as predict takes it -> (n_p, r, r) float64; pass
        it to ``reconstruct_std(cov=...)`` for the uncertainty map of the field.

        This is NOT what predict's second output holds: the reference defines  Ar_sigma = |P sigma_y0|  (:874), the image of
        the deviation vector, whereas the coefficient deviations are  sqrt(diag(P P^T)) -- and the covariance is in general
        not diagonal, so a correct map needs all of it.

        All-zero uncertainties give a zero matrix (Ar_sigma = 0 there, :868-870); uncertainties that are zero for only some
        sensors raise np.linalg.LinAlgError as predict does.  method='COLS' raises NotImplementedError: bounds that are
        active change the covariance.  Host-sized work (s x r per vector), np.linalg.pinv with predict's rcond."""
        if isinstance(y, np.ndarray):
            y = [y]
        Theta = np.asarray(self.Theta, dtype=np.float64)
        for yi in y:
            if Theta.shape[0] != yi.shape[0]:
                raise ValueError('The number of rows of Theta does not match the number'
                                 ' of rows of y.')
            if yi.shape[1] != 3:
                raise ValueError('The y array has the wrong number of columns. y has'
                                 ' to have dimensions (s,3).')
        if self.method == 'COLS':
            raise NotImplementedError("coefficient_covariance: method='COLS' is not covered -- active bounds change the "
                                      'covariance of the constrained solution.')
        if self.method != 'OLS':
            raise NotImplementedError('The prediction method selected has not been '
                                      'implemented yet')
        cov = np.zeros((len(y), self.r, self.r))
        for i, yi in enumerate(y):
            yi = np.asarray(yi, dtype=np.float64)
            if not np.any(yi[:, 1]):
                continue
            sig0 = yi[:, 1] / self._scl_f[yi[:, 2].astype('int')]
            if not np.all(np.isfinite(sig0)) or np.any(sig0 == 0):
                raise np.linalg.LinAlgError('SVD did not converge')           # W = diag(1/0): what np.linalg.pinv raises
            P = np.linalg.pinv(Theta / sig0[:, None], rcond=self._PINV_RCOND)
            cov[i] = P @ P.T
        return cov

    #: train(method='COLS') (_cols.py): a row counts as violated when it exceeds its scaled limit by more than cols_tol
    #: (scaled units, i.e. multiples of X_scl); at most cols_rows_per_round (<= 256) rows join a vector's working set per
    #: sweep; predict raises RuntimeError rather than return an unconverged vector after cols_max_rounds sweeps or
    #: beyond cols_max_rows working rows.
    cols_tol = 1e-9
    cols_rows_per_round = 64
    cols_max_rounds = 60
    cols_max_rows = 4000

    def predict(self, y):
        """Reference :822-901.  Returns (Ar, Ar_sigma), each (n_p, r).  method == 'COLS' (:880-892): constrained least
        squares by constraint generation (_cols.py); diagnostics in ``cols_info_``; an infeasible vector is a row of NaN."""
        if isinstance(y, np.ndarray):
            y = [y]
        for i in range(len(y)):
            if self.Theta.shape[0] != y[i].shape[0]:
                raise ValueError('The number of rows of Theta does not match the number'
                                 ' of rows of y.')
            if y[i].shape[1] != 3:
                raise ValueError('The y array has the wrong number of columns. y has'
                                 ' to have dimensions (s,3).')
        if self.method not in ('OLS', 'COLS'):
            raise NotImplementedError('The prediction method selected has not been '
                                      'implemented yet')
        if len(y) == 0:                                       # :863-864 allocate (0, r) and the loop never runs
            return np.zeros((0, self.r)), np.zeros((0, self.r))
        if self.method == 'COLS':
            from ._cols import predict_cols
            Ar, Ar_sigma = predict_cols(self, y)
        else:
            Ar, Ar_sigma, y0 = self._solve(y)
        self.cnt_vector = self._engine().to_host(self._d['cnt'])
        self.scl_vector = self._scl_f[np.asarray(y[-1])[:, 2].astype('int')]
        return Ar, Ar_sigma

    # ------------------------------------------------------------------ sensors fused with a Gaussian prior
    @staticmethod
    def _prior_operand(eng, A, n_p, core_ndim):
        """A prior operand of assimilate whose shape has been checked -> float64, (n_p,) + core, on the device: an operand of
        ``core_ndim`` dimensions is broadcast over the vectors.  Host input is uploaded, a device tensor stays where it is."""
        if hasattr(A, 'is_cuda'):
            if A.dtype != eng.torch.float64:
                raise ValueError(f'a prior given on the device must be float64, got {A.dtype}.')
            return A.expand((n_p,) + tuple(A.shape)) if A.dim() == core_ndim else A
        A = np.asarray(A, dtype=np.float64)
        return eng.to_device(np.broadcast_to(A, (n_p,) + A.shape) if A.ndim == core_ndim else A)

    def assimilate(self, y, prior_mean, prior_sigma=None, *, prior_factor=None, prior_cov=None, to_host=True):
        """The Bayesian update of a Gaussian prior on the coefficients with sensor readings, on the device: the operating
        point supplies  a ~ N(a0, S0)  (``GPR.predict``), the sensors correct it.  In the scaled units predict works in,
        y0 = (y[:, 0] - cnt) / scl,  sig0 = y[:, 1] / scl,  R = diag(sig0^2):

            cov = (Theta^T R^-1 Theta + S0^-1)^-1,      a = a0 + cov Theta^T R^-1 (y0 - Theta a0)

        computed in the scaled form that never inverts S0: with S0 = C C^T, B = W Theta C, W = diag(1 / sig0),
        H' = I + B^T B = L' L'^T,  z = H'^-1 B^T W (y0 - Theta a0),  a = a0 + C z,  F = C L'^-T,  cov = F F^T.  H' is
        positive definite for any sensor count: fewer sensors than modes need no pseudo-inverse and no rank decision.

        ``y``             what predict takes: (s, 3) or a list of n_p of them.  Every uncertainty y[:, 1] must be finite and
                          non-zero (ValueError): an update needs a noise level; predict's "all zero means W = I" has no
                          meaning here.
        ``prior_mean``    (n_p, r), or (r,) for every vector.
        exactly one of
        ``prior_sigma``   (n_p, r) or (r,), finite and >= 0: independent deviations, the orientation of GPR.predict's
                          ``A_sigma``.  A coefficient with sigma 0 returns its prior mean bit for bit.
        ``prior_factor``  (n_p, r, q) or (r, q), 1 <= q <= r: S0 = C C^T -- e.g. the third output of an earlier call.
        ``prior_cov``     (n_p, r, r) or (r, r): factored on the host as reconstruct_std(cov=) does, same ValueError for a
                          matrix that is not positive semi-definite.
        Means, sigmas and factors may be device tensors (GPR.predict(to_host=False), assimilate(to_host=False)).

        -> (Ar (n_p, r), Ar_std (n_p, r) = sqrt(diag(cov)), factor (n_p, r, q) with cov = factor factor^T): host arrays, or
        the three device tensors with ``to_host=False``.  ``factor`` goes into ``reconstruct_std(factor=...)`` or into the
        next call as ``prior_factor``.  Diagnostics per vector in ``assimilate_info_``: status (0 ok), cond =
        (max L'_jj / min L'_jj)^2, chi2 = res^T (Theta S0 Theta^T + R)^-1 res with res = y0 - Theta a0 (about ``dof`` = s
        when prior and sensors agree), logdet = log det(Theta S0 Theta^T + R), dof, prior (the form that was used).
        method='COLS' and more than 128 modes raise NotImplementedError.  Sharded objects: Theta, cnt and the scales are
        replicated, every rank computes the same result, no collective."""
        if isinstance(y, np.ndarray):
            y = [y]
        if 'Theta' not in self._d or 'cnt' not in self._d:
            raise AttributeError("assimilate needs a trained object: call train(C) first ('SPR' object has no attribute 'C')")
        s, r = self._d['Theta'].shape
        for yi in y:
            if np.ndim(yi) != 2 or yi.shape[0] != s:
                raise ValueError('The number of rows of Theta does not match the number'
                                 ' of rows of y.')
            if yi.shape[1] != 3:
                raise ValueError('The y array has the wrong number of columns. y has'
                                 ' to have dimensions (s,3).')
        if self.method == 'COLS':
            raise NotImplementedError("assimilate: method='COLS' is not covered -- active bounds change the posterior.")
        if self.method != 'OLS':
            raise NotImplementedError('The prediction method selected has not been '
                                      'implemented yet')
        if r > SPR_MAX_R:
            raise NotImplementedError(f'assimilate takes bases of up to {SPR_MAX_R} modes, this one has {r}; keep fewer modes.')
        if sum(x is not None for x in (prior_sigma, prior_factor, prior_cov)) != 1:
            raise ValueError('assimilate takes exactly one of prior_sigma, prior_factor and prior_cov.')
        if self._d['cnt'].shape[0] != s:
            raise ValueError(f'operands could not be broadcast together: y has {s} rows, '
                             f"C has {self._d['cnt'].shape[0]}")
        eng = self._engine()
        n_p = len(y)
        form = 'sigma' if prior_sigma is not None else 'factor' if prior_factor is not None else 'cov'
        # the readings, on the host: feature ids as predict checks and wraps them, uncertainties that can weigh a sensor
        Yh = np.stack([np.asarray(yi, dtype=np.float64) for yi in y]) if n_p else np.zeros((0, s, 3))
        fid = Yh[:, :, 2].astype('int')                                   # as predict indexes X_scl with it
        n_rows = self._n_global
        bad = (fid * self.n_points >= n_rows) | (fid * self.n_points < -n_rows)
        if bad.any():
            k = int(fid.ravel()[np.argmax(bad.ravel())]) * self.n_points
            raise IndexError(f'index {k} is out of bounds for axis 0 with size {n_rows}')
        if (fid < 0).any():
            Yh[:, :, 2] = np.where(fid < 0, fid + self.n_features, fid)
            fid = Yh[:, :, 2].astype('int')
        sig0 = Yh[:, :, 1] / self._scl_f[fid]
        if not np.all(np.isfinite(sig0)) or np.any(sig0 == 0):
            raise ValueError('assimilate needs a sensor uncertainty y[:, 1] that is finite and not zero for every sensor: '
                             'the update weighs the sensors against the prior by it.')
        # the prior: shapes first (nothing is uploaded for an operand that is refused, or for an empty batch)
        want = {'mean': f'({n_p}, {r}) or ({r},)', 'sigma': f'({n_p}, {r}) or ({r},)',
                'factor': f'({n_p}, {r}, q) or ({r}, q) with 1 <= q <= {r}', 'cov': f'({n_p}, {r}, {r}) or ({r}, {r})'}
        given = {'mean': prior_mean, 'sigma': prior_sigma, 'factor': prior_factor, 'cov': prior_cov}
        tails = {'mean': (r,), 'sigma': (r,), 'factor': (r, None), 'cov': (r, r)}
        q = r
        for name in ('mean', form):
            shape, tail = tuple(np.shape(given[name])), tails[name]
            core = shape[1:] if len(shape) == len(tail) + 1 and shape[0] == n_p else shape
            if not (len(core) == len(tail) and all(t is None or t == k for t, k in zip(tail, core))
                    and (name != 'factor' or 1 <= core[1] <= r)):
                raise ValueError(f'prior_{name} must have shape {want[name]}, got {shape}.')
            if name == 'factor':
                q = core[1]
        if n_p == 0:
            self.assimilate_info_ = dict(status=np.zeros(0, dtype=int), cond=np.zeros(0), chi2=np.zeros(0), logdet=np.zeros(0),
                                         dof=np.zeros(0, dtype=int), prior=form)
            if to_host:
                return np.zeros((0, r)), np.zeros((0, r)), np.zeros((0, r, q))
            return eng.empty((0, r)), eng.empty((0, r)), eng.empty((0, r, q))
        S = L = None
        if form == 'sigma':
            ok = eng.torch.isfinite(prior_sigma) & (prior_sigma >= 0) if hasattr(prior_sigma, 'is_cuda') else \
                np.isfinite(np.asarray(prior_sigma, dtype=np.float64)) & (np.asarray(prior_sigma, dtype=np.float64) >= 0)
            if not bool(ok.all()):
                raise ValueError('prior_sigma must be finite and >= 0.')
            S = self._prior_operand(eng, prior_sigma, n_p, 1)
        elif form == 'factor':
            L = self._prior_operand(eng, prior_factor, n_p, 2)
        else:
            Lh = self._cov_factors(np.asarray(prior_cov, dtype=np.float64).reshape(-1, r, r))
            if Lh is None:                                    # every covariance is zero: the prior comes back as it is
                S = eng.zeros((n_p, r))
            else:
                L, q = eng.to_device(np.broadcast_to(Lh, (n_p,) + Lh.shape[1:])), Lh.shape[2]
        a0 = self._prior_operand(eng, prior_mean, n_p, 1)
        Ar, Ar_std, F, info_d, _ = eng.assimilate(self._d['Theta'], self._d['cnt'], self._d['scale'], eng.to_device(Yh), a0,
                                                  S=S, L=L)
        info = np.asarray(eng.to_host(info_d))
        self.assimilate_info_ = dict(status=info[:, 0].astype(int), cond=info[:, 1].copy(), chi2=info[:, 2].copy(),
                                     logdet=info[:, 3].copy(), dof=np.full(n_p, s), prior=form)
        if np.any(info[:, 0] != 0):
            import warnings
            warnings.warn('assimilate: the factorisation broke down for vector(s) '
                          f'{np.flatnonzero(info[:, 0] != 0).tolist()} (a prior or a reading that is not finite?); see '
                          'assimilate_info_["status"].', RuntimeWarning, stacklevel=2)
        if not to_host:
            return Ar, Ar_std, F
        return np.array(eng.to_host(Ar)), np.array(eng.to_host(Ar_std)), np.array(eng.to_host(F))
