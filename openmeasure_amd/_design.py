"""Oversampled sensor placement by sequential optimal design (no counterpart in the reference: its 'qr' placement returns
exactly r sensors, :740, and GEM's picks beyond r - 1 are decided by unseeded noise): greedy D- or A-optimal additions to a
set of sensors, one sweep of csrc/design.hip over the basis per added sensor.  Methods of SPR (a mixin: rom.SPR inherits
them).

With M = Theta^T W Theta (+ diag(ridge)) the information matrix of the sensors placed so far, W = diag(1 / sigma^2) in the
scaled units predict() works in, the candidate row u with weight w is scored from z = M^-1 u, d = u^T z, q = z^T z:

    'D'  w d                  det(M + w u u^T) = det M (1 + w d): the largest gain of log det M
    'A'  w q / (1 + w d)      the Sherman-Morrison drop of trace M^-1 = trace(coefficient_covariance)
"""
from __future__ import annotations

import numpy as np

from ._lib import SPR_MAX_R
from ._placement import _check_mask

_COND_MAX = 1e12      # augment_placement(ridge=0): the start must give an information matrix better conditioned than this


def _inverse(M):
    """-> (B = M^-1 symmetric, log det M, trace M^-1) from a Cholesky factorisation of M (host, f64, r <= 128)."""
    L = np.linalg.cholesky(M)
    Li = np.linalg.solve(L, np.eye(M.shape[0]))
    B = Li.T @ Li
    return 0.5 * (B + B.T), 2.0 * float(np.sum(np.log(np.diag(L)))), float(np.sum(Li * Li))


class DesignPlacement:
    """augment_placement, placement_gain and calc_type='dopt' | 'aopt' of SPR.optimal_placement (mixed into rom.SPR)."""

    # ------------------------------------------------------------------ arguments
    def _design_engine(self):
        eng = self._engine()
        if not hasattr(eng, 'design_sweep'):
            raise NotImplementedError("this engine has no 'design_sweep' (csrc/design.hip); there is no CPU fallback.")
        return eng

    def _design_start(self, start):
        """start=None | integer rows | one-hot ndarray | OneHotRows -> int64 global rows"""
        from .rom import OneHotRows
        n = self._n_global
        if start is None:
            rows = np.asarray(self.sensors_, dtype=np.int64)  # AttributeError before any placement
        elif isinstance(start, OneHotRows):
            if start.ndim != 2 or start.shape[1] != n:
                raise ValueError(f'start: a one-hot matrix needs {n} columns')
            rows = start.rows.copy()
        else:
            a = np.asarray(start)
            if a.ndim == 2:
                if a.shape[1] != n or not (np.all((a == 0) | (a == 1)) and np.all(a.sum(axis=1) == 1)):
                    raise ValueError(f'start: a 2-D array must be a one-hot matrix with {n} columns')
                rows = np.argmax(a, axis=1).astype(np.int64)
            elif a.ndim == 1 and (a.size == 0 or np.issubdtype(a.dtype, np.integer)):
                rows = a.astype(np.int64)
            else:
                raise ValueError('start: integer global rows, a one-hot matrix or a OneHotRows')
        if rows.size and (rows.min() < 0 or rows.max() >= n):
            raise IndexError(f'start: sensor row outside [0, {n})')
        return rows

    def _design_weights(self, noise):
        """noise (n_features,) standard deviations in physical units -> w_f = (X_scl_f / sigma_f)^2, the W^2 of predict"""
        F = self.n_features
        if noise is None:
            return np.ones(F), False
        noise = np.asarray(noise, dtype=np.float64)
        if noise.shape != (F,):
            raise ValueError(f'noise must have one standard deviation per feature, shape ({F},); got {noise.shape}')
        if not np.all(np.isfinite(noise)) or np.any(noise <= 0):
            raise ValueError('noise: the standard deviations must be finite and positive')
        self._fitted('scale', 'X_scl')
        return (np.asarray(self._scl_f, dtype=np.float64)[:F] / noise) ** 2, True

    @staticmethod
    def _design_ridge(ridge, r):
        rd = np.asarray(ridge, dtype=np.float64)
        if rd.ndim == 0:
            rd = np.full(r, float(rd))
        if rd.shape != (r,) or not np.all(np.isfinite(rd)) or np.any(rd < 0):
            raise ValueError(f'ridge: a non-negative scalar or ({r},) prior precisions')
        return rd

    def _design_rows(self, eng, Ur_d, rows):
        """the rows `rows` (global) of the basis, each of which lives on one rank -> host (k, r)"""
        k = len(rows)
        if k == 0:
            return np.zeros((0, Ur_d.shape[1]))
        ip, ix, v = self._csr_device(None, (np.arange(k + 1), rows, np.ones(k)))
        rows_d, _ = eng.measure_csr(ip, ix, v, Ur_d, self._row0, self._fitted('rowmean', 'X_cnt'))
        return np.asarray(eng.to_host(self._all_reduce(rows_d)), dtype=np.float64)

    def _design_matrix(self, eng, Ur_d, rows, wts, ridge):
        U0 = self._design_rows(eng, Ur_d, rows)
        w0 = wts[np.minimum(rows // self.n_points, self.n_features - 1)] if len(rows) else np.zeros(0)
        return np.diag(ridge) + (U0 * w0[:, None]).T @ U0

    def _design_regular(self, M, ridge, what):
        """B, logdet, trace of M^-1 -- or the ValueError that names ``ridge``"""
        hint = (f'{what}: the information matrix of the start sensors is singular or ill-conditioned (fewer than r = '
                f'{M.shape[0]} independent sensors, as after a GEM placement): pass ridge > 0 (prior precisions, '
                '1 / prior_sigma**2 of assimilate)')
        if not np.any(ridge > 0):
            with np.errstate(all='ignore'):
                cond = np.linalg.cond(M) if np.all(np.isfinite(M)) else np.inf
            if not cond < _COND_MAX:
                raise ValueError(hint + f'; cond(M) = {cond:.3g}')
        try:
            return _inverse(M)
        except np.linalg.LinAlgError:
            raise ValueError(hint) from None

    # ------------------------------------------------------------------ augment_placement
    def augment_placement(self, n_sensors, criterion='D', start=None, mask=None, d_min=0., noise=None, ridge=0.):
        """Greedy D- or A-optimal additions to the sensors ``start`` until there are ``n_sensors``: the answer to "I can
        afford s > r noisy probes, where do the extra ones go?".  Returns C with n_sensors rows (as optimal_placement does);
        the ordered rows are in ``sensors_``, the relative lead of every pick over its runner-up in ``pivot_gap_`` (0 for the
        start rows), the sweeps over the basis in ``pivot_sweeps_``, and ``design_info_`` holds criterion, weights, logdet and
        trace_inv after every sensor (n_added + 1 entries), the winning score of every pick (gain: w d for 'D' -- the gain
        of log det M is log1p of it --, the drop of trace M^-1 for 'A'), cond at start and end and cov = the final M^-1.

        start   the sensors to keep: None = ``sensors_`` of the last placement, integer global rows, a one-hot ndarray or a
                OneHotRows (already installed probes).  n_sensors == len(start) returns the start with zero sweeps.
        noise   None or (n_features,) sensor standard deviations in physical units: weights (X_scl_f / sigma_f)^2.
        ridge   scalar or (r,) prior precisions added to the diagonal of M (1 / prior_sigma**2 of assimilate: Bayesian
                D/A-optimality).  With ridge = 0 the start must give cond(M) < 1e12 -- a GEM placement needs a ridge.
        mask, d_min   rows outside the mask, the start rows, every pick, and rows closer than d_min to a start row or a pick
                are never chosen (the rule of optimal_placement('gem')).  The basis is not modified.
        Per added sensor: M^-1 afresh from a Cholesky factorisation on the host (M accumulates w u u^T from the records'
        rows: no Sherman-Morrison drift), one sweep, one record downloaded; sharded objects all-gather the records."""
        self._flush_deferred()
        if criterion not in ('D', 'A'):
            raise ValueError(f"criterion must be 'D' or 'A', got {criterion!r}")
        Ur_d = self._fitted('Ur', 'Ur')
        n_loc, r = Ur_d.shape
        if r > SPR_MAX_R:
            raise NotImplementedError(f'augment_placement: r = {r} retained modes exceed the {SPR_MAX_R} the design sweep '
                                      'is built for; keep fewer modes.')
        eng = self._design_engine()
        t = eng.torch
        if not isinstance(n_sensors, (int, np.integer)):
            raise TypeError(f"'{type(n_sensors).__name__}' object cannot be interpreted as an integer")
        n_sensors = int(n_sensors)
        rows0 = self._design_start(start)
        k0 = len(rows0)
        if n_sensors < k0:
            raise ValueError(f'augment_placement: n_sensors = {n_sensors} is the TOTAL and must not be smaller than the '
                             f'{k0} start sensors')
        wts, weighted = self._design_weights(noise)
        rd = self._design_ridge(ridge, r)
        xyz = None
        if mask is not None:
            mask = np.asarray(mask)
            _check_mask(mask, n_loc)
        if d_min > 0:
            xyz = np.asarray(self.xyz, dtype=np.float64)
            if xyz.ndim != 2 or xyz.shape[0] != self.n_points or not 1 <= xyz.shape[1] <= 3:
                raise ValueError('augment_placement with d_min > 0 needs xyz of shape (n_points, 1..3).')
        if n_sensors == k0:                                   # nothing to add: no sweep and no device work
            self.sensors_ = rows0
            self.pivot_gap_ = np.zeros(k0)
            self.pivot_sweeps_ = 0
            self.__dict__.pop('design_info_', None)
            C = self._one_hot(rows0, self._n_global)
            self._placed = (C, rows0)
            return C
        mask_d = eng.to_device(mask.astype(np.uint8), dtype=t.uint8) if mask is not None else None
        xyz_d = eng.to_device(xyz) if xyz is not None else None
        M = self._design_matrix(eng, Ur_d, rows0, wts, rd)
        B, logdet, tr = self._design_regular(M, rd, 'augment_placement')
        cond0 = float(np.linalg.cond(M))

        # the race: a negative entry of `alive` takes a row out (the pivoting state's convention, kept by qr_exclude)
        piv = np.full(n_sensors, -1, dtype=np.int64)
        piv[:k0] = rows0
        st = dict(Ur=Ur_d, n=n_loc, r=r, row0=self._row0, nrm=eng.zeros((n_loc,)), piv=eng.to_device(piv, dtype=t.int64))
        alive = st['nrm']

        def leave(rows):
            loc = np.asarray(rows, dtype=np.int64) - self._row0
            loc = loc[(loc >= 0) & (loc < n_loc)]
            if loc.size:
                alive[t.as_tensor(loc, dtype=t.int64, device=alive.device)] = -1.0

        if mask_d is not None:
            eng.qr_exclude(st, mask=mask_d, n_points=self.n_points)
        leave(rows0)
        if xyz_d is not None:
            for j0 in range(0, k0, eng.qr_batch):
                eng.qr_exclude(st, xyz=xyz_d, n_points=self.n_points, j0=j0, nq=min(eng.qr_batch, k0 - j0), d_min=float(d_min))
        wfeat_d = eng.to_device(wts) if weighted else None
        logdets, traces, gains, gaps = [logdet], [tr], [], []
        sweeps = 0
        for j in range(k0, n_sensors):
            rec = eng.design_sweep(Ur_d, self._row0, self.n_points, self.n_features, eng.to_device(B), wfeat_d, alive,
                                   criterion)
            sweeps += 1
            recs = np.asarray(eng.to_host(self._all_gather(rec)), dtype=np.float64)   # (ranks, r + 3)
            order = np.lexsort((recs[:, 1], -recs[:, 0]))     # value descending, then global row (as _gem_ridge_phase)
            best = recs[order[0]]
            if best[1] < 0 or not best[0] > -np.inf:
                raise RuntimeError('augment_placement: no admissible row left for the remaining sensors (mask / d_min too '
                                   'strict)')
            g = int(best[1])
            runner = max([best[2]] + [recs[i, 0] for i in order[1:]])
            gaps.append((best[0] - runner) / best[0] if best[0] > 0 and np.isfinite(runner) else
                        (np.inf if best[0] > 0 else 0.0))
            gains.append(float(best[0]))
            u = best[3:3 + r]
            M = M + wts[min(g // self.n_points, self.n_features - 1)] * np.outer(u, u)
            try:
                B, logdet, tr = _inverse(M)
            except np.linalg.LinAlgError:
                raise ValueError('augment_placement: the information matrix lost positive definiteness; pass a larger '
                                 'ridge') from None
            logdets.append(logdet)
            traces.append(tr)
            piv[j] = g
            st['piv'][j] = g
            leave([g])
            if xyz_d is not None:
                eng.qr_exclude(st, xyz=xyz_d, n_points=self.n_points, j0=j, nq=1, d_min=float(d_min))
        self.sensors_ = piv
        self.pivot_gap_ = np.concatenate([np.zeros(k0), np.asarray(gaps, dtype=np.float64)])
        self.pivot_sweeps_ = sweeps
        self.design_info_ = dict(criterion=criterion, weights=wts.copy(), logdet=np.asarray(logdets), trace_inv=np.asarray(traces),
                                 gain=np.asarray(gains), cond=(cond0, float(np.linalg.cond(M))), cov=B)
        C = self._one_hot(piv, self._n_global)
        self._placed = (C, piv)
        return C

    # ------------------------------------------------------------------ placement_gain
    def placement_gain(self, criterion='D', sensors=None, noise=None, ridge=0., to_host=True):
        """The (n,) score of every row as the NEXT sensor after ``sensors`` (None: ``sensors_``), to be plotted like a field:
        the score map of one design sweep with no exclusions (see augment_placement for criterion, noise and ridge)."""
        self._flush_deferred()
        if criterion not in ('D', 'A'):
            raise ValueError(f"criterion must be 'D' or 'A', got {criterion!r}")
        if self._dist():
            raise NotImplementedError('placement_gain of a sharded object is not covered.')
        Ur_d = self._fitted('Ur', 'Ur')
        n_loc, r = Ur_d.shape
        if r > SPR_MAX_R:
            raise NotImplementedError(f'placement_gain: r = {r} retained modes exceed the {SPR_MAX_R} the design sweep is '
                                      'built for; keep fewer modes.')
        eng = self._design_engine()
        rows = self._design_start(sensors)
        wts, weighted = self._design_weights(noise)
        rd = self._design_ridge(ridge, r)
        M = self._design_matrix(eng, Ur_d, rows, wts, rd)
        B, _, _ = self._design_regular(M, rd, 'placement_gain')
        scores = eng.empty((n_loc,))
        eng.design_sweep(Ur_d, self._row0, self.n_points, self.n_features, eng.to_device(B),
                         eng.to_device(wts) if weighted else None, None, criterion, scores=scores)
        return eng.to_host(scores) if to_host else scores

    # ------------------------------------------------------------------ optimal_placement('dopt' | 'aopt')
    def _placement_design(self, calc_type, n_sensors, mask, d_min):
        """The 'qr' placement (r sensors, including its in-place masking of the basis), then greedy D / A additions."""
        r = self._fitted('Ur', 'Ur').shape[1]
        if r > SPR_MAX_R:
            raise NotImplementedError(f"optimal_placement('{calc_type}'): r = {r} retained modes exceed the {SPR_MAX_R} the "
                                      'design sweep is built for; keep fewer modes.')
        self._design_engine()
        if not isinstance(n_sensors, (int, np.integer)):
            raise TypeError(f"'{type(n_sensors).__name__}' object cannot be interpreted as an integer")
        if n_sensors < r:
            raise ValueError(f"optimal_placement('{calc_type}'): n_sensors = {n_sensors} is smaller than the r = {r} sensors "
                             "of the 'qr' placement it starts from")
        self.optimal_placement('qr', mask=mask)
        sweeps = self.pivot_sweeps_
        C = self.augment_placement(int(n_sensors), 'D' if calc_type == 'dopt' else 'A', mask=mask, d_min=d_min)
        self.pivot_sweeps_ += sweeps
        return C
