"""CoKriging: operating parameters -> high-fidelity field from two sets of simulations (reference: CoKriging,
cokriging.py:19-144): many cheap low-fidelity (LF) runs on one mesh and a few expensive high-fidelity (HF) runs on another.

``CoKriging(X_train_l, X_train_u, Y_train_lf_l, Y_train_lf_u, Y_train_hf_l, xyz_lf, xyz_hf, n_features)`` with the reference's
surface -- ``manifold_alignment``, ``fit``, ``predict`` -- plus ``predict_latent``.  ``manifold_alignment`` is two ``ROM.fit`` on
the device and a Procrustes alignment of the two POD score manifolds on the host (the meshes may differ: nothing is
interpolated); ``fit`` trains, per latent dimension, a two-level co-kriging model on the device: one workgroup per dimension
runs the whole Adam loop of a level in one launch (csrc/cokriging.hip), two launches in all; ``predict`` is two launches and
``ROM.reconstruct`` / ``ROM.reconstruct_std`` -- the basis never leaves the device.

The model every number here follows (per latent dimension; d parameters; level 0 = LF on all n0 = n_u + n_l points ordered
UNLINKED FIRST, LINKED LAST -- the nested design; level 1 = HF on the n_l linked points):

    normalisation (``normalize``): X by its mean and population std over the n0 points; y by the mean and std of
    y_best = [LF targets at the unlinked points, HF targets at the linked points]; a zero std becomes 1.
    one level:  theta_c = 10^v_c,  R_ij = exp(-sum_c theta_c (x_ic - x_jc)^2) + nugget delta_ij,
        F = [1, x] at level 0 (``regr_type='constant'``: [1]);  F = [y0(x), 1, x] at level 1, y0 the LF DATA at the linked
        points, its coefficient is rho;  n > p' columns is required (ValueError);
        beta = (F^T R^-1 F)^-1 F^T R^-1 y,  gamma = R^-1 (y - F beta),  sigma2 = (y - F beta)^T gamma / (n - p'),
        loss(theta) = [ (n - p') log sigma2 + log det R ] / n        (the concentrated likelihood, not GPR's marginal one)
    training: Adam on v (beta 0.9 / 0.999, eps 1e-8, bias correction, step ``lr``): evaluate, e = |loss - loss_old|, step, clip v
        to [log10 thetaL, log10 thetaU], stop when e <= ``tol`` or after ``max_iter`` evaluations.  Defaults: theta0 = 0.5 per
        coordinate, thetaL = 1e-5, thetaU = 50, tol = 1e-6, lr = 0.1, max_iter = 1000.  ``theta`` given: no optimisation.
    prediction at x*:  f* = [1, x*] / [mu0(x*), 1, x*],  r*_i = exp(-sum theta_c (x*_c - x_ic)^2),
        mu = f*^T beta + r*^T gamma,  u = F^T R^-1 r* - f*,  mse_own = max(sigma2 (1 - r*^T R^-1 r* + u^T (F^T R^-1 F)^-1 u), 0),
        MSE = sigma_rho^2 MSE0 + mse_own1,  sigma_rho^2 = rho^2 + sigma2_1 [(F1^T R1^-1 F1)^-1]_00   (Le Gratiet's recursion),
        un-normalised: mu y_std + y_mean, MSE y_std^2.

Departures from the reference, on purpose:

* PAIRING.  The reference stacks the LF snapshots linked first (:57), the parameters unlinked first (:110), and pairs them as
  they are (:118): LF scores meet the wrong operating points.  Here the aligned LF scores are reordered to unlinked-first
  before training, so every target belongs to its parameter row and the design is nested.  ``Zr_aligned`` itself keeps the
  reference's column order (linked first, as the snapshots were stacked).
* VARIANCE.  The reference returns ``unscale_data(Ur_hf @ Z_mse)`` (:136, :142): a variance pushed through a signed basis with
  the mean field added, which changes with LAPACK's column signs.  Here the second return of ``predict`` is the per-cell
  VARIANCE of the field, ``reconstruct_std(sqrt(Z_mse).T)**2``; ``predict_latent`` gives ``(Z_pred, Z_mse)`` for anything else.
* NUGGET.  The default is ``nugget = 1e-10`` (an attribute): with a nugget of 10 eps the LF level's R of a smooth noise-free
  case reached a condition number of 1e16, did not converge in 1000 evaluations and gave a meaningless MSE.
* OPTIMISER.  Adam on log10 theta instead of COBYLA; ``initial_range`` (COBYLA's first step) is accepted and stored only.
* openmdao's ``MultiFiCoKriging`` was not available to run against: the model is the one written above, pinned by the NumPy
  restatement in tests/test_cokriging_host.py; agreement of the TRAINED numbers with openmdao is unpinned.

Not built (NotImplementedError): ``regr_type`` other than 'constant' / 'linear', ``rho_regr`` other than 'constant', more than
two fidelity levels, more than 8 parameters, more than 800 training points, sharded inputs."""
from __future__ import annotations

import numpy as np

from ._lib import SPR_GP_MAX_D, SPR_GP_MAX_M
from .rom import ROM, DeviceMatrix

REGR_TYPES = ('constant', 'linear')
STATUS_TEXT = {1: 'a pivot of R is not positive', 2: 'a pivot of R is not finite', 3: 'the trend matrix F^T R^-1 F is singular',
               4: 'sigma2 is not positive and finite'}


class CKRecord:
    """What is kept of one latent dimension's trained model on the host, level 0 (LF) and level 1 (HF) in that order:
    ``theta`` (2, d), ``beta`` (two arrays: the trend coefficients; at level 1 the first is rho), ``rho``, ``sigma2`` (2,),
    ``iterations`` (2,) (evaluations of the training loop), ``loss`` (2,), ``status`` (2,) (0: trained)."""

    def __init__(self, theta, beta, sigma2, iterations, loss, status):
        self.theta = np.array(theta, dtype=np.float64)
        self.beta = [np.array(b, dtype=np.float64) for b in beta]
        self.rho = float(self.beta[1][0])
        self.sigma2 = np.array(sigma2, dtype=np.float64)
        self.iterations = np.array(iterations, dtype=np.int64)
        self.loss = np.array(loss, dtype=np.float64)
        self.status = np.array(status, dtype=np.int64)

    def __repr__(self):
        return (f'CKRecord(theta={np.array2string(self.theta, precision=6, separator=", ")}, rho={self.rho:.6g}, '
                f'sigma2={self.sigma2.tolist()}, iterations={self.iterations.tolist()}, loss={self.loss.tolist()}, '
                f'status={self.status.tolist()})')


class CoKriging:
    """Multi-fidelity POD co-kriging (reference: CoKriging, cokriging.py:19-144); the module docstring has the model and the
    departures.  The Y matrices may be ndarrays, device tensors or ``DeviceMatrix``; ``engine=`` as for ROM."""

    def __init__(self, X_train_l, X_train_u, Y_train_lf_l, Y_train_lf_u, Y_train_hf_l, xyz_lf, xyz_hf, n_features, engine=None,
                 *, shard=None):
        if shard is not None:
            raise NotImplementedError('sharded co-kriging is not part of this implementation.')
        self.X_train_l = X_train_l            # linked parameters
        self.X_train_u = X_train_u            # unlinked parameters
        self.Y_train_lf_l = Y_train_lf_l      # linked LF data
        self.Y_train_lf_u = Y_train_lf_u      # unlinked LF data
        self.Y_train_hf_l = Y_train_hf_l      # linked HF data
        self.xyz_lf = xyz_lf
        self.xyz_hf = xyz_hf
        self.n_features = n_features
        self.n_linked = X_train_l.shape[0]
        self.n_unlinked = X_train_u.shape[0]
        self.n_latent = 0
        self.scale_type = 'std'
        self.regr_type = 'linear'
        self.rho_regr = 'constant'
        self.normalize = True
        self.theta = None
        self.theta0 = None
        self.thetaL = None
        self.thetaU = None
        self.initial_range = 0.3              # COBYLA's first step in the reference: stored only
        self.tol = 1e-6
        self.nugget = 1e-10
        self.lr = 0.1
        self.max_iter = 1000
        self._eng = engine
        self._d = {}                          # device-resident state of fit()
        if (Y_train_lf_l.shape[1] != self.n_linked) or (Y_train_hf_l.shape[1] != self.n_linked):   # :44-48
            raise ValueError('The number of linked conditions does not correspond to the number of columns of '
                             'Y_train_lf_l or Y_train_hf_l')
        if Y_train_lf_u.shape[1] != self.n_unlinked:                                                # :49-53
            raise ValueError('The number of unlinked conditions does not correspond to the number of columns of '
                             'Y_train_lf_u')

    # ------------------------------------------------------------------ plumbing
    def _engine(self):
        if self._eng is None:
            from .engine import HipEngine
            self._eng = HipEngine()
        return self._eng

    def _ck_engine(self):
        eng = self._engine()
        for name in ('ck_train', 'ck_predict'):
            if not hasattr(eng, name):
                raise NotImplementedError(f"this engine has no '{name}' (csrc/cokriging.hip); there is no CPU fallback.")
        return eng

    @staticmethod
    def _device_block(eng, Y):
        """a snapshot block as a device tensor: a DeviceMatrix' tensor, a device tensor as it is, an ndarray uploaded (float32
        stays float32: storage only, see DeviceMatrix)"""
        if isinstance(Y, DeviceMatrix):
            return Y.tensor
        if isinstance(Y, eng.torch.Tensor):
            return Y
        Y = np.asarray(Y)
        return eng.to_device(Y, dtype=eng.torch.float32 if Y.dtype == np.float32 else None)

    def _check_model(self):
        if self.regr_type not in REGR_TYPES:
            raise NotImplementedError(f"regr_type={self.regr_type!r} is not part of this implementation: one of {REGR_TYPES}.")
        if self.rho_regr != 'constant':
            raise NotImplementedError(f"rho_regr={self.rho_regr!r} is not part of this implementation: only 'constant'.")
        d = np.shape(self.X_train_l)[1]
        if d > SPR_GP_MAX_D:
            raise NotImplementedError(f'{d} parameters exceed the {SPR_GP_MAX_D} the kernel keeps a theta for.')
        n0 = self.n_linked + self.n_unlinked
        if n0 > SPR_GP_MAX_M:
            raise NotImplementedError(f'{n0} training points exceed the {SPR_GP_MAX_M} the in-kernel Cholesky is built for.')

    # ------------------------------------------------------------------ :55-107
    def manifold_alignment(self, select_modes='variance', n_modes_hf=99, n_modes_lf=99):
        """Two ``ROM.fit(scale_type=self.scale_type, ...)`` on the device, then the Procrustes alignment of the LF scores onto
        the HF scores over the linked columns (reference :84-102, host, float64).  Sets ``rom_hf``, ``rom_lf``, ``Sigma_hf``,
        ``Sigma_lf``, ``r_hf``, ``r_lf``, ``n_latent`` (= r_hf), ``Zr_aligned`` (n_latent, n_l + n_u; columns linked first, as the
        snapshots are stacked), ``Zr_hf`` (r_hf, n_l), ``sr``, ``Qr``, and ``Ur_hf``: the HF basis, which stays on the device."""
        eng = self._engine()
        if 'Y_lf' not in self._d:                              # the two LF blocks are concatenated once, on the device
            lf_l, lf_u = self._device_block(eng, self.Y_train_lf_l), self._device_block(eng, self.Y_train_lf_u)
            if lf_l.dtype != lf_u.dtype:
                lf_l, lf_u = lf_l.to(eng.torch.float64), lf_u.to(eng.torch.float64)
            self._d['Y_lf'] = eng.torch.cat([lf_l, lf_u], dim=1).contiguous()
            self._d['Y_hf'] = self._device_block(eng, self.Y_train_hf_l)
        for k in ('model_list', 'cokriging_info_'):
            self.__dict__.pop(k, None)
        for k in ('X', 'fit0', 'fit1', 'v0', 'v1', 'srho2'):
            self._d.pop(k, None)
        self.rom_hf = ROM(DeviceMatrix(self._d['Y_hf']), self.n_features, self.xyz_hf, engine=eng)
        self.rom_lf = ROM(DeviceMatrix(self._d['Y_lf']), self.n_features, self.xyz_lf, engine=eng)
        self.rom_hf.fit(scale_type=self.scale_type, select_modes=select_modes, n_modes=n_modes_hf)
        self.rom_lf.fit(scale_type=self.scale_type, select_modes=select_modes, n_modes=n_modes_lf)
        self.Sigma_hf = np.asarray(self.rom_hf.S_, dtype=np.float64)
        self.Sigma_lf = np.asarray(self.rom_lf.S_, dtype=np.float64)
        self._align()

    def _align(self):
        """reference :78-107 from the two fitted ROMs' scores ``Ar`` (host, float64)"""
        for k in ('model_list', 'cokriging_info_'):
            self.__dict__.pop(k, None)
        Zr_hf = np.array(self.rom_hf.Ar, dtype=np.float64).T          # the reference's Zr: (r, snapshots)
        Zr_lf = np.array(self.rom_lf.Ar, dtype=np.float64).T
        self.r_hf, self.r_lf = Zr_hf.shape[0], Zr_lf.shape[0]
        if self.r_lf < self.r_hf:                                     # :84-86
            Zr_lf = np.concatenate([Zr_lf, np.zeros((self.r_hf - self.r_lf, Zr_lf.shape[1]))], axis=0)
        Zr_lf_l = Zr_lf[:, :self.n_linked]                            # :88
        Z0r_hf = Zr_hf - np.mean(Zr_hf, axis=1, keepdims=True)        # :91-97
        Z0r_lf_l = Zr_lf_l - np.mean(Zr_lf_l, axis=1, keepdims=True)
        Ur, Sigmar, Vr_t = np.linalg.svd(Z0r_lf_l @ Z0r_hf.T, full_matrices=False)   # :99
        self.sr = np.sum(Sigmar) / np.trace(Z0r_lf_l @ Z0r_lf_l.T)
        self.Qr = Vr_t.T @ Ur.T
        self.Zr_aligned = self.sr * self.Qr @ Zr_lf                   # :102
        self.n_latent = self.Zr_aligned.shape[0]
        self.Zr_hf = Zr_hf

    @property
    def Ur_hf(self):
        """the HF basis (n_hf_rows, r_hf) as a device tensor"""
        return self.rom_hf._fitted('Ur', 'Ur_hf')

    # ------------------------------------------------------------------ :109-119
    def _level_theta(self, value, level, d):
        """theta / theta0 of a level: a scalar, d values, or one such entry per level -> (d,)"""
        a = value
        if isinstance(a, (list, tuple)) and len(a) == 2 and not (d == 2 and all(np.ndim(x) == 0 for x in a)):
            a = a[level]
        a = np.asarray(a, dtype=np.float64)
        if a.ndim == 0:
            a = np.full(d, float(a))
        if a.shape != (d,) or not np.all(np.isfinite(a)) or np.any(a <= 0):
            raise ValueError(f'theta / theta0 must be positive: a scalar, {d} values, or a pair of those (one per level).')
        return a

    def fit(self):
        """Normalisation on the host, then two launches: level 0 (LF, all n0 points, unlinked first) for all latent
        dimensions, level 1 (HF, linked points) with the LF targets at the linked points as the rho column.  Sets
        ``model_list`` (one CKRecord per latent dimension) and ``cokriging_info_`` (dict; every value is a pair, level 0 and
        level 1: theta (n_latent, d), iterations, loss, e, status, sigma2 (n_latent,), beta (n_latent, p'), grad (n_latent, d),
        rho (None, (n_latent,))).  A status other than 0 raises numpy.linalg.LinAlgError."""
        if not hasattr(self, 'Zr_aligned'):
            raise AttributeError('The function manifold_alignment has to be called before calling fit.')
        self._check_model()
        eng = self._ck_engine()
        X_l, X_u = np.asarray(self.X_train_l, dtype=np.float64), np.asarray(self.X_train_u, dtype=np.float64)
        X = np.concatenate([X_u, X_l], axis=0)                        # :110
        n_u, n_l, (n0, d), r = self.n_unlinked, self.n_linked, X.shape, self.n_latent
        regr = self.regr_type
        p0 = 1 + (d if regr == 'linear' else 0)
        if n0 <= p0 or n_l <= p0 + 1:
            raise ValueError(f'a level needs more points than trend columns: {n0} LF points for {p0}, {n_l} HF points for '
                             f'{p0 + 1}.')
        max_iter, lr, tol, nugget = int(self.max_iter), float(self.lr), float(self.tol), float(self.nugget)
        if max_iter < 0 or not (lr > 0 and np.isfinite(lr)) or not (tol >= 0 and np.isfinite(tol)) or not (
                nugget >= 0 and np.isfinite(nugget)):
            raise ValueError('fit needs max_iter >= 0, a positive finite lr, and a non-negative finite tol and nugget.')
        thetaL = 1e-5 if self.thetaL is None else float(np.min(self.thetaL))
        thetaU = 50.0 if self.thetaU is None else float(np.max(self.thetaU))
        if not (0 < thetaL <= thetaU and np.isfinite(thetaU)):
            raise ValueError('fit needs 0 < thetaL <= thetaU, both finite.')
        v_lo, v_hi = float(np.log10(thetaL)), float(np.log10(thetaU))
        start = self.theta if self.theta is not None else (0.5 if self.theta0 is None else self.theta0)
        if self.theta is not None:
            max_iter = 0                                              # theta given: factor there, no optimisation
        v_start = [np.tile(np.log10(self._level_theta(start, lev, d)), (r, 1)) for lev in (0, 1)]
        # the pairing fix: column j of the targets belongs to row j of X (unlinked first, linked last)
        Y0 = np.concatenate([self.Zr_aligned[:, n_l:], self.Zr_aligned[:, :n_l]], axis=1)     # (r, n0)
        Y1 = np.asarray(self.Zr_hf, dtype=np.float64)                                        # (r, n_l)
        if not (np.all(np.isfinite(X)) and np.all(np.isfinite(Y0)) and np.all(np.isfinite(Y1))):
            raise ValueError('fit: the parameters or the scores have entries that are not finite.')
        if self.normalize:
            self.X_mean, self.X_std = X.mean(axis=0), X.std(axis=0)
            y_best = np.concatenate([Y0[:, :n_u], Y1], axis=1)
            self.y_mean, self.y_std = y_best.mean(axis=1), y_best.std(axis=1)
            self.X_std[self.X_std == 0.0] = 1.0
            self.y_std[self.y_std == 0.0] = 1.0
        else:
            self.X_mean, self.X_std = np.zeros(d), np.ones(d)
            self.y_mean, self.y_std = np.zeros(r), np.ones(r)
        Xn = (X - self.X_mean) / self.X_std
        Y0n = ((Y0 - self.y_mean[:, None]) / self.y_std[:, None]).T   # (n0, r)
        Y1n = ((Y1 - self.y_mean[:, None]) / self.y_std[:, None]).T   # (n_l, r)
        X_d, Y0_d, Y1_d = eng.to_device(Xn), eng.to_device(Y0n), eng.to_device(Y1n)
        train = dict(nugget=nugget, v_lo=v_lo, v_hi=v_hi, lr=lr, max_iter=max_iter, tol=tol)
        v0, fit0, info0, _ = eng.ck_train(X_d, Y0_d, None, regr, eng.to_device(v_start[0]), **train)
        v1, fit1, info1, _ = eng.ck_train(X_d[n_u:], Y1_d, Y0_d[n_u:], regr, eng.to_device(v_start[1]), **train)
        infos = [eng.to_host(info0), eng.to_host(info1)]
        for lev, info in enumerate(infos):
            bad = np.flatnonzero(info[:, 3] != 0)
            if len(bad):
                why = '; '.join(f'dimension {k + 1}: {STATUS_TEXT.get(int(info[k, 3]), "status %d" % info[k, 3])}' for k in bad)
                raise np.linalg.LinAlgError(f'fit: level {lev} ({"LF" if lev == 0 else "HF"}) could not be factored with '
                                            f'nugget = {nugget:g} ({why}); a larger nugget regularises R.')
        vs = [eng.to_host(v0), eng.to_host(v1)]
        betas = [np.array(eng.to_host(fit0['beta'])), np.array(eng.to_host(fit1['beta']))]
        s2 = [np.array(eng.to_host(fit0['sigma2'])), np.array(eng.to_host(fit1['sigma2']))]
        srho2 = fit1['beta'][:, 0] ** 2 + fit1['sigma2'] * fit1['Ginv'][:, 0, 0]
        self._d.update(X=X_d, v0=v0, fit0=fit0, v1=v1, fit1=fit1, srho2=srho2)
        self.cokriging_info_ = dict(
            theta=[10.0 ** v for v in vs], iterations=[i[:, 0].astype(np.int64) for i in infos], loss=[i[:, 1].copy() for i in infos],
            e=[i[:, 2].copy() for i in infos], status=[i[:, 3].astype(np.int64) for i in infos], sigma2=s2, beta=betas,
            grad=[i[:, 4:4 + d].copy() for i in infos], rho=[None, betas[1][:, 0].copy()], nugget=nugget, n_train=(n0, n_l),
            converged=[i[:, 2] <= tol for i in infos])
        c = self.cokriging_info_
        self.model_list = [CKRecord([c['theta'][0][k], c['theta'][1][k]], [betas[0][k], betas[1][k]], [s2[0][k], s2[1][k]],
                                    [c['iterations'][0][k], c['iterations'][1][k]], [c['loss'][0][k], c['loss'][1][k]],
                                    [c['status'][0][k], c['status'][1][k]]) for k in range(r)]

    # ------------------------------------------------------------------ :122-144
    def _check_n_truncated(self, n_truncated):
        if n_truncated is None:
            return self.n_latent
        if not (isinstance(n_truncated, (int, np.integer)) and 0 < n_truncated <= self.n_latent):
            raise ValueError(f'n_truncated must be an integer in 1..{self.n_latent}, got {n_truncated!r}.')
        return int(n_truncated)

    def predict_latent(self, X_test, n_truncated=None, *, to_host=True):
        """HF POD scores and their mean squared error at the parameters ``X_test`` (n_test, d) -> (Z_pred, Z_mse), each
        (n_truncated, n_test) (``to_host=False``: device tensors).  Two launches: level 0, then level 1 with level 0's mean as the
        rho regressor; the two MSEs combine by Le Gratiet's recursion (module docstring)."""
        if not hasattr(self, 'model_list'):
            raise AttributeError('The function fit has to be called before calling predict.')
        nt = self._check_n_truncated(n_truncated)
        eng = self._ck_engine()
        X_test = np.asarray(X_test, dtype=np.float64)
        if X_test.ndim < 2:
            X_test = X_test[np.newaxis, :]
        d = len(self.X_mean)
        if X_test.ndim != 2 or X_test.shape[1] != d:
            raise ValueError(f'the parameters must have shape (n_test, {d}), got {X_test.shape}.')
        Xs = (X_test - self.X_mean) / self.X_std
        if not np.all(np.isfinite(Xs)):
            raise ValueError('predict: the normalised parameters have entries that are not finite.')
        if X_test.shape[0] == 0:
            return (np.zeros((nt, 0)), np.zeros((nt, 0))) if to_host else (eng.empty((nt, 0)), eng.empty((nt, 0)))
        s = self._d
        Xs_d = eng.to_device(Xs)
        m0, mse0 = eng.ck_predict(s['X'], Xs_d, None, self.regr_type, s['v0'], s['fit0'])
        m1, mse1 = eng.ck_predict(s['X'][self.n_unlinked:], Xs_d, m0, self.regr_type, s['v1'], s['fit1'])
        y_mean, y_std = eng.to_device(self.y_mean), eng.to_device(self.y_std)
        Z_pred = (m1 * y_std + y_mean).T[:nt].contiguous()
        Z_mse = ((s['srho2'] * mse0 + mse1) * (y_std * y_std)).T[:nt].contiguous()
        if not to_host:
            return Z_pred, Z_mse
        return np.array(eng.to_host(Z_pred)), np.array(eng.to_host(Z_mse))

    def predict(self, X_test, n_truncated=None):
        """The HF field and its per-cell VARIANCE at ``X_test`` (n_test, d) -> (Y_pred, Y_var), each (n_hf_rows, n_test):
        ``rom_hf.reconstruct`` of the predicted scores and ``rom_hf.reconstruct_std(sqrt(Z_mse).T)**2`` (the scores of the
        truncated dimensions count as 0 with no uncertainty)."""
        Z_pred, Z_mse = self.predict_latent(X_test, n_truncated, to_host=False)
        eng = self._engine()
        nt, n_test = Z_pred.shape
        A, S = eng.zeros((n_test, self.n_latent)), eng.zeros((n_test, self.n_latent))
        A[:, :nt] = Z_pred.T
        S[:, :nt] = Z_mse.T.sqrt()
        Y_pred = self.rom_hf.reconstruct(A)
        Y_var = self.rom_hf.reconstruct_std(S) ** 2
        return Y_pred, Y_var
