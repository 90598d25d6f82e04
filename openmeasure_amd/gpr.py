"""GPR: operating parameters -> field, exact Gaussian processes on the POD coefficients (reference: GPR, gpr.py:165-675).

``GPR(ROM)`` with the reference's surface -- constructor, ``scale_GPR_data``, ``fit``, ``train``, ``predict``, ``update`` --
for ``gpr_type='SingleTask'``: one exact GP per retained mode with a constant mean, one of four stationary kernels and
homoscedastic Gaussian noise with the floor 1e-4.  The default is the reference's: a single lengthscale and no output scale;
``GPKernel(name, ard=True, scale=True)`` is gpytorch's ``ScaleKernel(MaternKernel(2.5, ard_num_dims=d))`` idiom, one
lengthscale per operating parameter and a prior variance that is trained.  The r GPs are trained together on the device: one
workgroup per mode runs the whole Adam loop, convergence test included, in one launch (csrc/gp.hip); ``predict`` is one launch
for all modes and test points.  The model every number here follows:

    raw = (raw_l, raw_n, mu), all 0 at the start;  l = softplus(raw_l),  s2 = softplus(raw_n) + 1e-4,
    K = k(D / l) + s2 I,  D = Euclidean distances of P0 (clamped below at 1e-15),  alpha = K^-1 (y - mu),
    loss = [ (y - mu)^T alpha / 2 + log det K / 2 + (m / 2) log 2 pi ] / m,
    Adam (beta 0.9 / 0.999, eps 1e-8, bias correction): evaluate, e = |loss - loss_old|, step, stop when e <= rel_error
    or after max_iter evaluations (the reference's loop, :230-247).

With a flagged GPKernel (L = d with ``ard`` else 1, S = 1 with ``scale`` else 0, n_par = L + S + 2):

    raw = (raw_l[0..L-1], [raw_o], raw_n, mu), all 0 at the start;  l_c = softplus(raw_l[c]),  o = softplus(raw_o) or 1,
    z_i = P0[i, :] / l coordinate by coordinate,  t_ij = max(|z_i - z_j|_2, 1e-15),  K = o k(t) + s2 I,  the same loss and loop;
    predict: mean = mu + o k*.alpha,  var = max(o - o^2 k*^T K^-1 k*, 0) + s2.

Measured coefficients go back into the GPs with their own noise (``update(P_meas, Ar, Ar_std, retrain=True)`` or
``fixed_noise=True``; the reference's FixedNoiseGaussianLikelihood, :660-675), for either kernel form:

    n_i = w_i s2 + V[i, q] for mode q,  K = o k(t) + diag(n),  the same loss;
    d loss / d raw_n = sigmoid(raw_n) sum_i w_i (K^-1_ii - alpha_i^2) / 2m,  the other components unchanged in form;
    w = 1, V = 0 on the points of fit() (the learned noise), w = 0, V = (A_sigma_new / Sigma_r)**2 on the new ones.

The reference instead gives the original points the train-mode prior deviation ``Vr_sigma`` (about 1) as fixed noise; here
they keep the learned s2.  ``predict`` adds s2 at the test point in every case (latent + simulation noise), never V.

This is gpytorch's exact marginal log likelihood for that model as read from its code; gpytorch itself was not available to
run against, so agreement of the NUMBERS with the reference is unpinned.  The oracle is the NumPy restatement
in tests/test_gpr_host.py (tests/test_gpr_ard_host.py for the flagged kernels, tests/test_gpr_noise_host.py for the per-point
noise).

``gpr_type='MultiTask'`` (the reference's batch of r GPs under a MultitaskGaussianLikelihood, :65-106, :466-483): the model
above per mode q with its own raw_q, its noise entry now the TASK noise raw_t, plus ONE shared raw_g, all 0 at the start:

    s2_q = (softplus(raw_t_q) + 1e-4) + (softplus(raw_g) + 1e-4),  K_q = o_q k(t) + s2_q I,  loss_q as above,
    LOSS = (1 / r) sum_q loss_q  (ExactMarginalLogLikelihood divides by the m r entries of the target);
    own parameters of q: the single-task gradient / r;  d LOSS / d raw_g = sigmoid(raw_g) (1 / r) sum_q sum_i (K_q^-1_ii - alpha_qi^2) / 2m;
    ONE Adam loop over the r n_par + 1 values, the reference's loop and stopping test on LOSS;
    predict: mean = mu_q + o_q k*.alpha_q,  var = max(o_q - o_q^2 k*^T K_q^-1 k*, 0) + s2_q, s2_q as the last evaluation used it.

On the device the loop is a chain of launches driven by a phase word (csrc/gp.hip, "multitask"; ``engine.gp_train_mt``).
``models`` / ``likelihoods`` are lists of ONE ``GPMultiTaskRecord``; ``update`` keeps the learned noises on all points (the
reference installs no fixed-noise likelihood there); ``fixed_noise``, ``append`` and ``forget`` are not built for it.  The oracle
is tests/test_gpr_multitask_host.py; parity of the trained numbers with gpytorch is unpinned here too.

Not built (NotImplementedError): ``PIGPR``, correlated tasks, gpytorch objects as ``mean`` / ``kernel`` /
``likelihood``, ARD over more than 8 parameters, priors on hyper-parameters, ``update(retrain=True)`` without
``A_sigma_new``, a fixed noise for the training set of ``train``, removing single points from a factored state (``forget``
factors again), the cvxpy ``problem_dict`` of ``predict``, more than 800 training points (gpytorch's ``max_cholesky_size``: up to
there the reference is an exact Cholesky GP too).

Several updates accumulate with ``update(..., append=True)``: the new points join the data held now, and the factor's inverse
X = L^-1 kept beside K^-1 gains k rows in O(m^2 k) per mode instead of a new O(m^3) factorisation (the ``update`` docstring;
the NumPy restatement is gp_append_oracle in tests/test_gpr_append_host.py)."""
from __future__ import annotations

import numpy as np

from ._lib import SPR_GP_MAX_APPEND, SPR_GP_MAX_D, SPR_GP_MAX_M
from .rom import ROM

KERNELS = ('matern52', 'matern32', 'matern12', 'rbf')
NOISE_FLOOR = 1e-4


def _softplus(x):
    return np.logaddexp(0.0, x)


class GPKernel:
    """A kernel of ``GPR.train``: ``name`` (one of KERNELS), ``ard`` (one lengthscale per operating parameter instead of one
    shared), ``scale`` (a trained output scale o, K = o k + s2 I, instead of the prior variance 1).  Immutable, hashable,
    picklable.  ``GPKernel('matern52', ard=True, scale=True)`` stands for gpytorch's
    ``ScaleKernel(MaternKernel(2.5, ard_num_dims=d))``; with both flags False it is the plain string."""
    __slots__ = ('name', 'ard', 'scale')

    def __init__(self, name='matern52', ard=False, scale=False):
        if not isinstance(name, str) or name not in KERNELS:
            raise ValueError(f'GPKernel: name must be one of {KERNELS}, got {name!r}')
        for k, v in (('name', name), ('ard', bool(ard)), ('scale', bool(scale))):
            object.__setattr__(self, k, v)

    def __setattr__(self, key, value):
        raise AttributeError('GPKernel is immutable')

    __delattr__ = __setattr__

    @property
    def flags(self):
        """bit 0: ARD, bit 1: output scale (the engine's and the library's encoding)"""
        return int(self.ard) | (int(self.scale) << 1)

    def n_par(self, d):
        return (d if self.ard else 1) + int(self.scale) + 2

    def __eq__(self, other):
        return isinstance(other, GPKernel) and (self.name, self.ard, self.scale) == (other.name, other.ard, other.scale)

    def __hash__(self):
        return hash((GPKernel, self.name, self.ard, self.scale))

    def __reduce__(self):
        return GPKernel, (self.name, self.ard, self.scale)

    def __repr__(self):
        return f'GPKernel({self.name!r}, ard={self.ard}, scale={self.scale})'


class GPRecord:
    """What is kept of one trained GP on the host: ``lengthscale``, ``noise``, ``mean`` (the constrained values), ``raw``
    (the unconstrained ones), ``iterations`` (evaluations of the training loop), ``loss`` (of the last of them),
    ``status`` (0: factorised), ``outputscale`` (1.0 without a scale).  Three raws (raw_l, raw_n, mu) by default; with ``ard`` /
    ``scale`` raw = (raw_l[0..L-1], [raw_o], raw_n, mu) and ``lengthscale`` is an ndarray of shape (L,) under ``ard``."""

    def __init__(self, raw, iterations, loss, status, ard=False, scale=False):
        self.raw = np.array(raw, dtype=np.float64)
        L = len(self.raw) - 2 - int(bool(scale))
        if L < 1 or (L != 1 and not ard):
            raise ValueError(f'GPRecord: {len(self.raw)} raw values do not fit ard={ard}, scale={scale}')
        self.lengthscale = np.asarray(_softplus(self.raw[:L])) if ard else float(_softplus(self.raw[0]))
        self.outputscale = float(_softplus(self.raw[L])) if scale else 1.0
        self.noise = float(_softplus(self.raw[-2]) + NOISE_FLOOR)
        self.mean = float(self.raw[-1])
        self.iterations = int(iterations)
        self.loss = float(loss)
        self.status = int(status)
        self._flagged = bool(ard or scale)

    def __repr__(self):
        if getattr(self, '_flagged', False):
            ls = np.array2string(np.atleast_1d(self.lengthscale), precision=6, separator=', ')
            return (f'GPRecord(lengthscale={ls}, outputscale={self.outputscale:.6g}, noise={self.noise:.6g}, '
                    f'mean={self.mean:.6g}, iterations={self.iterations}, loss={self.loss:.6g}, status={self.status})')
        return (f'GPRecord(lengthscale={self.lengthscale:.6g}, noise={self.noise:.6g}, mean={self.mean:.6g}, '
                f'iterations={self.iterations}, loss={self.loss:.6g}, status={self.status})')


class GPMultiTaskRecord:
    """What is kept of the r jointly trained GPs of ``gpr_type='MultiTask'`` on the host -- ONE record, the model and the
    likelihood of the reference's one-element lists: ``lengthscale`` (r,) or (r, d) under ``ard``, ``outputscale`` (r,; ones
    without a scale), ``task_noises`` (r,) and the shared ``noise`` (each with the floor 1e-4; mode q carries
    task_noises[q] + noise), ``mean`` (r,), ``raw`` (r, n_par) and ``raw_noise`` (the unconstrained values), ``iterations``
    (evaluations of the joint loop), ``loss`` (the joint loss of the last evaluation), ``status`` (r,; 0: factorised)."""

    def __init__(self, raw, raw_noise, iterations, loss, status, ard=False, scale=False):
        self.raw = np.array(raw, dtype=np.float64)
        if self.raw.ndim != 2:
            raise ValueError('GPMultiTaskRecord: raw must be (r, n_par)')
        L = self.raw.shape[1] - 2 - int(bool(scale))
        if L < 1 or (L != 1 and not ard):
            raise ValueError(f'GPMultiTaskRecord: {self.raw.shape[1]} raw values per mode do not fit ard={ard}, scale={scale}')
        self.raw_noise = float(np.asarray(raw_noise, dtype=np.float64).reshape(-1)[0])
        self.lengthscale = _softplus(self.raw[:, :L]) if ard else _softplus(self.raw[:, 0])
        self.outputscale = _softplus(self.raw[:, L]) if scale else np.ones(len(self.raw))
        self.task_noises = _softplus(self.raw[:, -2]) + NOISE_FLOOR
        self.noise = float(_softplus(self.raw_noise) + NOISE_FLOOR)
        self.mean = self.raw[:, -1].copy()
        self.iterations = int(iterations)
        self.loss = float(loss)
        self.status = np.asarray(status).astype(np.int64)

    def __repr__(self):
        a = lambda v: np.array2string(np.asarray(v), precision=6, separator=', ')
        return (f'GPMultiTaskRecord(tasks={len(self.raw)}, lengthscale={a(self.lengthscale)}, outputscale={a(self.outputscale)}, '
                f'task_noises={a(self.task_noises)}, noise={self.noise:.6g}, mean={a(self.mean)}, '
                f'iterations={self.iterations}, loss={self.loss:.6g}, status={a(self.status)})')


def _kurtosis(x):
    """scipy.stats.kurtosis(x, None): Fisher's definition, biased moments"""
    x = np.asarray(x, dtype=np.float64).ravel()
    c = x - x.mean()
    m2 = np.mean(c * c)
    return np.mean(c ** 4) / (m2 * m2) - 3.0


_GP_KEYS = ('gp_P0', 'gp_Y', 'gp_raw', 'gp_Kinv', 'gp_alpha',      # device state of a trained object (ROM._d: pickled as host arrays)
            'gp_raw_g', 'gp_s2')                                    # ... of a MultiTask object beside them


class GPR(ROM):
    """GPR-based ROM (reference: GPR, gpr.py:165-675); ``shard=`` / ``engine=`` as for ROM."""

    def __init__(self, X, n_features, xyz, P, gpr_type='SingleTask', shard=None, engine=None):
        super().__init__(X, n_features, xyz, shard=shard, engine=engine)
        self.P = P
        self.gpr_type = gpr_type
        if P.shape[0] != X.shape[1]:                           # :214-216
            raise Exception(f'The number of parameters ({P.shape[0]}) is different'
                            f' from the number of columns of X ({X.shape[1]})')

    # ------------------------------------------------------------------ :253-335
    def scale_GPR_data(self, P, scale_type):
        """Centre and scale the parameters column by column (host; P is (m, d) and tiny).  Sets ``P_cnt`` / ``P_scl``,
        returns ``P0 = (P - P_cnt) / P_scl``."""
        P = np.asarray(P)
        P_cnt = np.zeros_like(P)
        P_scl = np.zeros_like(P)
        for i in range(P.shape[1]):
            x = P[:, i]
            P_cnt[:, i] = np.mean(x)
            if scale_type == 'std':
                P_scl[:, i] = np.std(x)
            elif scale_type == 'none':
                P_scl[:, i] = 1.
            elif scale_type == 'pareto':
                P_scl[:, i] = np.sqrt(np.std(x))
            elif scale_type == 'vast':
                P_scl[:, i] = np.std(x) ** 2 / np.average(x)
            elif scale_type == 'range':
                P_scl[:, i] = np.max(x) - np.min(x)
            elif scale_type == 'level':
                P_scl[:, i] = np.average(x)
            elif scale_type == 'max':
                P_scl[:, i] = np.max(x)
            elif scale_type == 'variance':
                P_scl[:, i] = np.var(x)
            elif scale_type == 'median':
                P_scl[:, i] = np.median(x)
            elif scale_type == 'poisson':
                P_scl[:, i] = np.sqrt(np.average(x))
            elif scale_type == 'vast_2':
                P_scl[:, i] = (np.std(x) ** 2 * _kurtosis(x) ** 2) / np.average(x)
            elif scale_type == 'vast_3':
                P_scl[:, i] = (np.std(x) ** 2 * _kurtosis(x) ** 2) / np.max(x)
            elif scale_type == 'vast_4':
                P_scl[:, i] = (np.std(x) ** 2 * _kurtosis(x) ** 2) / (np.max(x) - np.min(x))
            elif scale_type == 'l2-norm':
                P_scl[:, i] = np.linalg.norm(x.flatten())
            else:
                raise NotImplementedError('The scaling method selected has not been '
                                          'implemented yet')
        self.P_cnt = P_cnt
        self.P_scl = P_scl
        return (P - P_cnt) / P_scl

    # ------------------------------------------------------------------ :337-402
    def fit(self, scaleX_type='std', scaleP_type='std', axis_cnt=1, select_modes='variance', n_modes=99, verbose=False,
            basis=None):
        """ROM.fit on the device plus the parameter scaling: leaves ``Ur``, ``Ar``, ``Sigma_r``, ``Vr``, ``r``, ``d``,
        ``P0`` (the scaled matrix ``X0`` of the reference is not kept on the host).  A trained state is dropped."""
        self.scaleX_type = scaleX_type
        self.scaleP_type = scaleP_type
        self.select_modes = select_modes
        self.n_modes = n_modes
        self.verbose = verbose
        for k in ('models', 'likelihoods', 'gpr_info_', 'Vr_sigma', 'append_info_', '_gp_X', '_gp_logdet', '_gp_state_of'):
            self.__dict__.pop(k, None)
        for k in _GP_KEYS:
            self._d.pop(k, None)
        ROM.fit(self, scale_type=scaleX_type, axis_cnt=axis_cnt, select_modes=select_modes, n_modes=n_modes, basis=basis)
        self.d = self.P.shape[1]
        self.P0 = GPR.scale_GPR_data(self, self.P, scaleP_type)

    # ------------------------------------------------------------------ :404-515
    def _check_gp_inputs(self, P0, Y, what):
        m = P0.shape[0]
        if m > SPR_GP_MAX_M:
            raise NotImplementedError(f'{what}: {m} training points exceed the {SPR_GP_MAX_M} an exact Cholesky GP is built '
                                      "for (gpytorch's max_cholesky_size; beyond it the reference is not an exact GP either).")
        if not np.all(np.isfinite(Y)):
            raise ValueError(f'{what}: Vr has entries that are not finite.')
        if not np.all(np.isfinite(P0)):
            raise ValueError(f'{what}: P0 has entries that are not finite.')

    def _gp_engine(self, flagged=False):
        return self._engine_with(('gp_train_ard', 'gp_predict_ard') if flagged else ('gp_train',), 'gp.hip')

    def _gp_kernel(self):
        """-> (name, GPKernel or None) of the trained object: the GPKernel only where it takes the ARD / scaled entry points"""
        k = self.kernel
        if isinstance(k, GPKernel):
            return k.name, (k if k.flags else None)
        return k, None

    @staticmethod
    def _raise_not_pd(status, what):
        bad = np.flatnonzero(status != 0)
        if len(bad):
            raise np.linalg.LinAlgError(f'{what}: the covariance matrix of mode(s) {(bad + 1).tolist()} is not positive '
                                        f'definite to working precision (status {status[bad].astype(int).tolist()}).')

    def train(self, mean=None, kernel=None, likelihood=None, max_iter=1000, rel_error=1e-5, lr=0.1, verbose=False):
        """Train one exact GP per retained mode on (P0, Vr[:, i]), all modes in one launch.

        ``mean`` / ``likelihood``: None only (constant mean, Gaussian noise with the floor 1e-4).  ``kernel``: None or
        'matern52' (the reference's default MaternKernel(2.5)), 'matern32', 'matern12', 'rbf', or a ``GPKernel`` -- with
        ``ard`` / ``scale`` the model of the module docstring (ARD over at most 8 parameters), with neither the string's path
        bit for bit.  Anything else raises NotImplementedError before any device work.  ``gpr_type='MultiTask'`` trains the
        jointly trained model instead (``_train_mt``: one record, joint ``gpr_info_``); over an engine without the multitask
        calls it is refused before any launch.
        With a flagged GPKernel the records' ``lengthscale`` is an ndarray (d,) under ``ard``, ``outputscale`` the trained
        scale, ``gpr_info_`` gains ``lengthscale`` (r, L) and ``outputscale`` (r,), its ``grad`` is (r, n_par), and
        ``Vr_sigma`` = sqrt(outputscale) per mode: the train-mode prior deviation sqrt(k(0)) again.

        -> (models, likelihoods): two lists of r host records (GPRecord; entry i of both lists is the same object: the
        noise belongs to the likelihood in the reference, the lengthscale and the mean to the model).  Sets ``models``,
        ``likelihoods``, ``gpr_info_`` (per-mode arrays: iterations, loss, e, status, grad, converged) and ``Vr_sigma``
        = ones (m, r): the reference stores the TRAIN-mode prior's standard deviation there (:249), which is sqrt(k(0)) = 1
        for these kernels -- read from the reference's code, not run.  ``verbose=True`` prints the reference's line per
        evaluation, from a trace buffer, after the launch.  A covariance matrix that is not positive definite to working
        precision raises numpy.linalg.LinAlgError.  Sharded objects: every rank trains the same GPs (Vr, P0 and the
        kernels are identical and deterministic), no collective."""
        if self.gpr_type == 'MultiTask':
            return self._train_mt(mean, kernel, likelihood, max_iter, rel_error, lr, verbose)
        if self.gpr_type != 'SingleTask':
            raise NotImplementedError(f"gpr_type='{self.gpr_type}' is not part of this implementation: only 'SingleTask' "
                                      "(one exact GP per mode) and 'MultiTask' (jointly trained, shared noise) are built.")
        if mean is not None or likelihood is not None:
            raise NotImplementedError('mean and likelihood must be None (constant mean, homoscedastic Gaussian noise): '
                                      'gpytorch objects are not part of this implementation.')
        gk = kernel if isinstance(kernel, GPKernel) and kernel.flags else None
        kern = 'matern52' if kernel is None else kernel.name if isinstance(kernel, GPKernel) else kernel
        if not isinstance(kern, str) or kern not in KERNELS:
            raise NotImplementedError(f'kernel must be None, one of {KERNELS} (one shared lengthscale, no output scale) or a '
                                      'GPKernel: gpytorch kernels are not part of this implementation.')
        if gk is not None and gk.ard and np.shape(self.P0)[1] > SPR_GP_MAX_D:
            raise NotImplementedError(f'train: ARD over {np.shape(self.P0)[1]} parameters exceeds the {SPR_GP_MAX_D} the '
                                      'kernel keeps a lengthscale for.')
        max_iter = int(max_iter)
        if max_iter < 0 or not (lr > 0 and np.isfinite(lr)) or not (rel_error >= 0 and np.isfinite(rel_error)):
            raise ValueError('train needs max_iter >= 0, a positive finite lr and a non-negative finite rel_error.')
        eng = self._gp_engine(gk is not None)
        P0 = np.ascontiguousarray(self.P0, dtype=np.float64)
        Vr = np.ascontiguousarray(self.Vr, dtype=np.float64)
        self._check_gp_inputs(P0, Vr, 'train')
        self.max_iter, self.rel_error, self.lr, self.verbose = max_iter, rel_error, lr, verbose
        self.mean, self.kernel, self.likelihood = None, (kernel if isinstance(kernel, GPKernel) else kern), None
        m, r = Vr.shape
        n_par = 3 if gk is None else gk.n_par(P0.shape[1])
        P0_d, Y_d = eng.to_device(P0), eng.to_device(Vr)
        if gk is None:
            raw, Kinv, alpha, info, trace = eng.gp_train(P0_d, Y_d, kern, eng.zeros((r, 3)), lr, max_iter, rel_error,
                                                         trace=bool(verbose))
        else:
            raw, Kinv, alpha, info, trace = eng.gp_train_ard(P0_d, Y_d, kern, gk.flags, eng.zeros((r, n_par)), lr, max_iter,
                                                             rel_error, trace=bool(verbose))
        info_h, raw_h = eng.to_host(info), eng.to_host(raw)
        self._raise_not_pd(info_h[:, 3], 'train')
        self._print_trace(eng, trace, info_h, n_par)
        self._d.update(gp_P0=P0_d, gp_Y=Y_d, gp_raw=raw, gp_Kinv=Kinv, gp_alpha=alpha)
        self._set_trained(gk, raw_h, info_h, m, n_par)
        return self.models, self.likelihoods

    def _print_trace(self, eng, trace, info_h, n_par):
        """the reference's line per evaluation (:240), from the trace buffer of a training launch"""
        if not self.verbose or trace is None:
            return
        tr, r = eng.to_host(trace), len(info_h)
        for i in range(r):
            for j in range(int(info_h[i, 0])):
                noise = _softplus(tr[i, j, n_par - 1]) + NOISE_FLOOR
                print(f'Iter {j+1:d}/{self.max_iter:d} - Mode: {i+1:d}/{r:d} - Loss: {tr[i, j, 0]:.2e} - '
                      f'Mean noise: {noise:.2e}')

    def _set_trained(self, gk, raw_h, info_h, m, n_par):
        """``models`` / ``likelihoods``, ``gpr_info_`` and ``Vr_sigma`` (m, r) from the host copies of a training launch"""
        r = len(raw_h)
        flag_kw = {} if gk is None else dict(ard=gk.ard, scale=gk.scale)
        models = [GPRecord(raw_h[i], info_h[i, 0], info_h[i, 1], info_h[i, 3], **flag_kw) for i in range(r)]
        self.gpr_info_ = dict(kernel=self.kernel, n_train=m, iterations=info_h[:, 0].astype(np.int64), loss=info_h[:, 1].copy(),
                              e=info_h[:, 2].copy(), status=info_h[:, 3].astype(np.int64), grad=info_h[:, 4:4 + n_par].copy(),
                              converged=info_h[:, 2] <= self.rel_error)
        self.Vr_sigma = np.ones((m, r))
        if gk is not None:
            self.gpr_info_.update(lengthscale=np.stack([np.atleast_1d(q.lengthscale) for q in models]),
                                  outputscale=np.array([q.outputscale for q in models]))
            self.Vr_sigma = self.Vr_sigma * np.sqrt(self.gpr_info_['outputscale'])
        self.models = models
        self.likelihoods = list(models)

    # ------------------------------------------------------------------ :517-601
    def _scale_params(self, P_star):
        P_star = np.asarray(P_star, dtype=np.float64)
        if P_star.ndim < 2:
            P_star = P_star[np.newaxis, :]
        if P_star.ndim != 2 or P_star.shape[1] != self.P_cnt.shape[1]:
            raise ValueError(f'the parameters must have shape (n_p, {self.P_cnt.shape[1]}), got {P_star.shape}.')
        return (P_star - self.P_cnt[0]) / self.P_scl[0]

    def predict(self, P_star, problem_dict=None, *, to_host=True):
        """POD coefficients and their standard deviation (observation noise included, as the reference's likelihood adds
        it) at the parameters ``P_star`` (n_p, d), or (d,) for one point.  -> (A_pred, A_sigma), each (n_p, r), column i
        multiplied by ``Sigma_r[i]``; ``to_host=False``: the two device tensors.  They feed the field and its uncertainty:

            A_pred, A_sigma = gpr.predict(P_star)
            X_rec = gpr.reconstruct(A_pred)            # (n, n_p)
            X_std = gpr.reconstruct_std(A_sigma)       # (n, n_p)

        (both methods take the device tensors of ``to_host=False`` as well).  ``problem_dict`` other than None raises
        NotImplementedError: the reference applies it to MultiTask models only."""
        if not hasattr(self, 'models'):
            raise AttributeError('The function fit has to be called '
                                 'before calling predict.')
        if problem_dict is not None:
            raise NotImplementedError('predict(problem_dict=...) is the constrained prediction of MultiTask models (cvxpy), '
                                      'which is not part of this implementation.')
        kern, gk = self._gp_kernel()
        mt = self.gpr_type == 'MultiTask'
        eng = self._mt_engine() if mt else self._gp_engine(gk is not None)
        P0_star = self._scale_params(P_star)
        if not np.all(np.isfinite(P0_star)):
            raise ValueError('predict: the scaled parameters have entries that are not finite.')
        r = self._mt_r() if mt else len(self.models)
        Sigma_r = np.asarray(self.Sigma_r, dtype=np.float64)
        if P0_star.shape[0] == 0:
            return (np.zeros((0, r)), np.zeros((0, r))) if to_host else (eng.empty((0, r)), eng.empty((0, r)))
        d_ = self._d
        if mt:
            mean, var = eng.gp_predict_mt(d_['gp_P0'], eng.to_device(P0_star), kern, self._mt_flags(), d_['gp_raw'], d_['gp_s2'],
                                          d_['gp_Kinv'], d_['gp_alpha'])
        elif gk is None:
            mean, var = eng.gp_predict(d_['gp_P0'], eng.to_device(P0_star), kern, d_['gp_raw'], d_['gp_Kinv'], d_['gp_alpha'])
        else:
            mean, var = eng.gp_predict_ard(d_['gp_P0'], eng.to_device(P0_star), kern, gk.flags, d_['gp_raw'], d_['gp_Kinv'],
                                           d_['gp_alpha'])
        if not to_host:
            S_d = eng.to_device(Sigma_r)
            return mean * S_d, var.sqrt() * S_d
        return eng.to_host(mean) * Sigma_r, np.sqrt(eng.to_host(var)) * Sigma_r

    def partial_fit(self, X_new, **kwargs):
        """Not built: the GPs are trained on ``P`` with one row per snapshot, and a batch that changes the basis brings
        no parameters with it.  ``update(P_new, A_new)`` conditions the GPs on new runs in the basis of fit()."""
        raise NotImplementedError('GPR.partial_fit is not part of this implementation: P has one row per snapshot, and new '
                                  'snapshots would change the basis under the trained GPs; use update(P_new, A_new).')

    # ------------------------------------------------------------------ :603-675
    def update(self, P_new, A_new, A_sigma_new=None, retrain=False, verbose=False, *, fixed_noise=False, append=False):
        """Condition the trained GPs on further data: the scaled ``P_new`` (k, d) and ``A_new / Sigma_r`` (k, r) are appended
        to (P0, Vr), the hyper-parameters are kept, K is factored again (one launch, no step).  As in the reference, the
        object's ``P0`` / ``Vr`` stay those of fit(): a second update replaces the data of the first.  The records' ``loss``
        and ``gpr_info_['loss']`` / ``['grad']`` / ``['n_train']`` become those of the new data at the kept hyper-parameters;
        ``iterations``, ``e`` and ``converged`` still describe the training.

        ``retrain=False, fixed_noise=False``: the new points carry the noise s2 learned for the simulations, and
        ``A_sigma_new`` only resizes ``Vr_sigma`` (zeros of the new shape, :654).

        ``fixed_noise=True``: the new points carry THEIR OWN noise, the standard deviations ``A_sigma_new`` (k, r; finite and
        >= 0, required) -- what ``SPR.predict`` / ``SPR.assimilate`` return beside the coefficients.  Per mode q the noise of
        point i is n_i = w_i s2 + V[i, q], K = o k(t) + diag(n): the m points of fit() keep the learned noise (w = 1, V = 0), the
        new ones get w = 0, V = (A_sigma_new / Sigma_r)**2 with no floor added (two contradictory exact points make K
        singular: LinAlgError).  ``Vr_sigma`` becomes zeros (m + k, r); ``gpr_info_`` gains ``noise_weight`` (m + k,) and
        ``fixed_noise`` (m + k, r), which a later plain update removes.

        ``retrain=True`` (implies ``fixed_noise``; the reference's FixedNoiseGaussianLikelihood branch, :660-675): the whole
        Adam loop of ``train`` on the concatenated data with that noise, in one launch, with ``lr`` / ``max_iter`` /
        ``rel_error`` of ``train``; the raw values start at the trained ones, Adam's moments, the previous loss and the
        counters afresh (the reference makes a new optimiser per call, :224).  d loss / d raw_n weighs its terms with w.
        ``models`` / ``likelihoods`` are new records, every array of ``gpr_info_`` is replaced, ``Vr_sigma`` = ones (m + k, r)
        sqrt(outputscale) as after ``train``; ``verbose`` prints the reference's line per evaluation.  Without
        ``A_sigma_new`` it raises NotImplementedError (the reference fails there too).

        On purpose not the reference's: there the ORIGINAL points get the train-mode prior deviation ``Vr_sigma`` (about 1) as
        their fixed noise and the training loop is handed the old likelihood; here they keep the learned s2.
        ``predict`` after either fixed-noise path adds s2 at the test point as before (latent + simulation noise), never V.

        ``append=True``: the new points are ADDED to the data the GPs are conditioned on now -- the simulations and every point
        of earlier updates, with the noise they came with -- instead of replacing the earlier updates, and K is not factored
        again: beside K^-1 the object keeps X = L^-1 of K = L L^T and log det K on the device, and k new points add k rows to X
        in O(m^2 k) per mode (``engine.gp_append``; more than 64 points go in consecutive slices of 64).  That state is built
        by one O(m^3) launch (``engine.gp_state``) when the object holds none that belongs to its current K^-1: after ``train``,
        after an ``append=False`` update, after a retrain, after ``forget`` and after unpickling; K^-1 and alpha then become that
        launch's (the same numbers to rounding).  With ``A_sigma_new`` the new points carry w = 0, V = (A_sigma_new /
        Sigma_r)**2 (the checks of ``fixed_noise``), without it the learned s2 (w = 1, V = 0).  ``Vr_sigma`` becomes zeros
        (m', r); ``gpr_info_`` gets ``n_train``, ``loss``, the accumulated ``noise_weight`` / ``fixed_noise`` and ``n_added``
        (points beyond those of fit()), its ``grad`` becomes NaN (no gradient is formed); the records' ``loss`` follows;
        ``append_info_`` holds per slice ``rows``, ``status`` (r,) and ``logdet`` (r,).  More than 800 points in all raise
        NotImplementedError before any launch: ``forget`` makes room.  A Schur complement that is not positive definite (a new
        exact point on top of an exact one) raises LinAlgError and leaves the data and the state as they were.
        ``append=True, retrain=True`` (needs ``A_sigma_new``) runs the training loop of ``retrain`` on the accumulated data
        with the accumulated w / V; the state is built again at the next append."""
        if self.gpr_type == 'MultiTask':
            return self._update_mt(P_new, A_new, A_sigma_new, retrain, verbose, fixed_noise, append)
        if append:
            return self._update_append(P_new, A_new, A_sigma_new, retrain, verbose)
        fixed = bool(fixed_noise or retrain)
        if fixed and A_sigma_new is None:
            if retrain:
                raise NotImplementedError('update(retrain=True) trains with a fixed-noise likelihood: pass A_sigma_new (k, r), the '
                                          'standard deviations of A_new (the Ar_sigma / Ar_std of SPR.predict / assimilate); '
                                          'retrain=False keeps the hyper-parameters.')
            raise ValueError('update(fixed_noise=True) needs A_sigma_new (k, r), the standard deviations of A_new.')
        if not hasattr(self, 'models'):
            raise AttributeError(f"'{type(self).__name__}' object has no attribute 'models'")
        self.verbose = verbose
        kern, gk = self._gp_kernel()
        eng = self._gp_engine(gk is not None)
        if fixed:
            self._engine_with(('gp_train_noise',), 'gp.hip')
        r = len(self.models)
        P0_new = self._scale_params(P_new)
        A_new = np.asarray(A_new, dtype=np.float64)
        if A_new.ndim < 2:
            A_new = A_new[np.newaxis, :]
        if A_new.shape != (P0_new.shape[0], r):
            raise ValueError(f'A_new must have shape ({P0_new.shape[0]}, {r}), got {A_new.shape}.')
        P0_tot = np.concatenate([np.asarray(self.P0, dtype=np.float64), P0_new], axis=0)
        Vr_tot = np.concatenate([np.asarray(self.Vr, dtype=np.float64), A_new / np.asarray(self.Sigma_r)], axis=0)
        self._check_gp_inputs(P0_tot, Vr_tot, 'update')
        if fixed:
            return self._update_fixed_noise(eng, kern, gk, P0_tot, Vr_tot, A_sigma_new, retrain)
        if A_sigma_new is not None:
            A_sigma_new = np.asarray(A_sigma_new, dtype=np.float64)
            self.Vr_sigma = np.zeros((self.Vr_sigma.shape[0] + A_sigma_new.shape[0], r))
        P0_d, Y_d = eng.to_device(P0_tot), eng.to_device(Vr_tot)
        if gk is None:
            raw, Kinv, alpha, info, _ = eng.gp_train(P0_d, Y_d, kern, self._d['gp_raw'], self.lr, 0, 0.0)
        else:
            raw, Kinv, alpha, info, _ = eng.gp_train_ard(P0_d, Y_d, kern, gk.flags, self._d['gp_raw'], self.lr, 0, 0.0)
        info_h = eng.to_host(info)
        self._raise_not_pd(info_h[:, 3], 'update')
        self._d.update(gp_P0=P0_d, gp_Y=Y_d, gp_Kinv=Kinv, gp_alpha=alpha)
        n_par = 3 if gk is None else info_h.shape[1] - 4
        self.gpr_info_.update(n_train=P0_tot.shape[0], loss=info_h[:, 1].copy(), grad=info_h[:, 4:4 + n_par].copy())
        for k in ('noise_weight', 'fixed_noise'):                # of an earlier fixed-noise update: this data has neither
            self.gpr_info_.pop(k, None)
        for i, rec in enumerate(self.models):
            rec.loss = float(info_h[i, 1])

    def _update_fixed_noise(self, eng, kern, gk, P0_tot, Vr_tot, A_sigma_new, retrain):
        """update(fixed_noise=True / retrain=True) behind the checks they share with the plain update: the concatenated data
        with the noise n_i = w_i s2 + V[i, q], factored at the kept hyper-parameters or trained from them (one launch)."""
        m_tot, r = Vr_tot.shape
        m = np.shape(self.Vr)[0]
        A_sigma_new = np.asarray(A_sigma_new, dtype=np.float64)
        if A_sigma_new.ndim < 2:
            A_sigma_new = A_sigma_new[np.newaxis, :]
        if A_sigma_new.shape != (m_tot - m, r):
            raise ValueError(f'A_sigma_new must have shape ({m_tot - m}, {r}), got {A_sigma_new.shape}.')
        if not (np.all(np.isfinite(A_sigma_new)) and np.all(A_sigma_new >= 0)):
            raise ValueError('A_sigma_new must be finite and >= 0: it holds standard deviations.')
        w = np.concatenate([np.ones(m), np.zeros(m_tot - m)])
        V = np.concatenate([np.zeros((m, r)), (A_sigma_new / np.asarray(self.Sigma_r, dtype=np.float64)) ** 2], axis=0)
        if not np.all(np.isfinite(V)):
            raise ValueError('update: (A_sigma_new / Sigma_r)**2 has entries that are not finite.')
        self._noise_launch(eng, kern, gk, P0_tot, Vr_tot, w, V, retrain)

    def _noise_launch(self, eng, kern, gk, P0_tot, Vr_tot, w, V, retrain):
        """one gp_train_noise launch on (P0_tot, Vr_tot) with the noise arrays w (m',) and V (m', r) -- a factorisation at the
        kept hyper-parameters, or the training loop from them -- and everything the object keeps of it"""
        m_tot, r = Vr_tot.shape
        flags = 0 if gk is None else gk.flags
        n_par = 3 if gk is None else gk.n_par(P0_tot.shape[1])
        P0_d, Y_d = eng.to_device(P0_tot), eng.to_device(Vr_tot)
        max_iter, tol = (self.max_iter, self.rel_error) if retrain else (0, 0.0)
        raw, Kinv, alpha, info, trace = eng.gp_train_noise(P0_d, Y_d, eng.to_device(w), eng.to_device(V), kern, flags,
                                                           self._d['gp_raw'], self.lr, max_iter, tol,
                                                           trace=bool(retrain and self.verbose))
        info_h = eng.to_host(info)
        self._raise_not_pd(info_h[:, 3], 'update')
        self._d.update(gp_P0=P0_d, gp_Y=Y_d, gp_Kinv=Kinv, gp_alpha=alpha)
        if retrain:
            self._print_trace(eng, trace, info_h, n_par)
            self._d['gp_raw'] = raw
            self._set_trained(gk, eng.to_host(raw), info_h, m_tot, n_par)
        else:
            self.gpr_info_.update(n_train=m_tot, loss=info_h[:, 1].copy(), grad=info_h[:, 4:4 + n_par].copy())
            for i, rec in enumerate(self.models):
                rec.loss = float(info_h[i, 1])
            self.Vr_sigma = np.zeros((m_tot, r))
        self.gpr_info_.update(noise_weight=w, fixed_noise=V)

    # ------------------------------------------------------------------ MultiTask (:65-106, :220-251, :657-663)
    def _mt_engine(self):
        eng = self._engine()
        for name in ('gp_train_mt', 'gp_predict_mt'):
            if not hasattr(eng, name):
                raise NotImplementedError(f"gpr_type='MultiTask' needs the engine's {name} (csrc/gp.hip); this engine has none, "
                                          'and there is no CPU fallback.')
        return eng

    def _mt_r(self):
        """modes of a trained MultiTask object: from the fit, ``models`` is a list of ONE record"""
        return int(self._d['gp_raw'].shape[0])

    def _mt_flags(self):
        return self.kernel.flags if isinstance(self.kernel, GPKernel) else 0

    def _train_mt(self, mean, kernel, likelihood, max_iter, rel_error, lr, verbose):
        """train() of ``gpr_type='MultiTask'``: the reference's batch of r GPs under a MultitaskGaussianLikelihood of rank 0 --
        a noise per task plus ONE shared noise, each with the floor 1e-4 -- and one ExactMarginalLogLikelihood over all m r
        targets: one loss, one Adam loop and one stopping test for the r n_par + 1 values (the module docstring).  ``kernel``
        as for SingleTask; the shared-lengthscale string kernels take the same device path with flags 0.
        -> (models, likelihoods): two lists of ONE GPMultiTaskRecord, the same object.  ``gpr_info_``: the joint
        ``iterations``, ``loss``, ``e``, ``converged``, ``grad`` (r n_par + 1,; the shared noise last), per-mode ``status``,
        ``n_train``, ``kernel``, and ``lengthscale`` / ``outputscale`` / ``task_noises`` / ``noise``.  ``verbose=True`` prints
        the reference's multitask line per evaluation (:243), with the shared noise."""
        eng = self._mt_engine()
        if mean is not None or likelihood is not None:
            raise NotImplementedError("MultiTask: mean and likelihood must be None (constant means, task noises plus one shared "
                                      'noise): gpytorch objects are not part of this implementation.')
        kern = 'matern52' if kernel is None else kernel.name if isinstance(kernel, GPKernel) else kernel
        if not isinstance(kern, str) or kern not in KERNELS:
            raise NotImplementedError(f'MultiTask: kernel must be None, one of {KERNELS} or a GPKernel: gpytorch kernels are not '
                                      'part of this implementation.')
        flags = kernel.flags if isinstance(kernel, GPKernel) else 0
        if flags & 1 and np.shape(self.P0)[1] > SPR_GP_MAX_D:
            raise NotImplementedError(f'MultiTask train: ARD over {np.shape(self.P0)[1]} parameters exceeds the {SPR_GP_MAX_D} '
                                      'the kernel keeps a lengthscale for.')
        max_iter = int(max_iter)
        if max_iter < 0 or not (lr > 0 and np.isfinite(lr)) or not (rel_error >= 0 and np.isfinite(rel_error)):
            raise ValueError('train needs max_iter >= 0, a positive finite lr and a non-negative finite rel_error.')
        P0 = np.ascontiguousarray(self.P0, dtype=np.float64)
        Vr = np.ascontiguousarray(self.Vr, dtype=np.float64)
        self._check_gp_inputs(P0, Vr, 'MultiTask train')
        self.max_iter, self.rel_error, self.lr, self.verbose = max_iter, rel_error, lr, verbose
        self.mean, self.kernel, self.likelihood = None, (kernel if isinstance(kernel, GPKernel) else kern), None
        r = Vr.shape[1]
        n_par = (P0.shape[1] if flags & 1 else 1) + (1 if flags & 2 else 0) + 2
        self._mt_launch(eng, kern, flags, P0, Vr, eng.zeros((r, n_par)), eng.zeros((1,)), True, 'train')
        return self.models, self.likelihoods

    def _mt_launch(self, eng, kern, flags, P0, Y, raw, raw_g, train, what):
        """one gp_train_mt call on (P0, Y) from (raw, raw_g) -- the joint loop, or (``train`` False) one evaluation at the kept
        values -- and everything the object keeps of it"""
        m, r = Y.shape
        n_par = int(raw.shape[1])
        NP = r * n_par + 1
        P0_d, Y_d = eng.to_device(P0), eng.to_device(Y)
        max_iter, tol = (self.max_iter, self.rel_error) if train else (0, 0.0)
        raw, raw_g, s2, Kinv, alpha, info, trace = eng.gp_train_mt(P0_d, Y_d, kern, flags, raw, raw_g, self.lr, max_iter, tol,
                                                                   trace=bool(train and self.verbose))
        info_h = eng.to_host(info)
        status = info_h[4 + NP:4 + NP + r]
        self._raise_not_pd(status, what)
        self._d.update(gp_P0=P0_d, gp_Y=Y_d, gp_Kinv=Kinv, gp_alpha=alpha, gp_s2=s2)
        if not train:
            self.gpr_info_.update(n_train=m, loss=float(info_h[1]), grad=info_h[4:4 + NP].copy())
            self.models[0].loss = float(info_h[1])
            return
        if self.verbose and trace is not None:
            tr = eng.to_host(trace)
            for j in range(int(info_h[0])):
                print(f'Iter {j+1:d}/{self.max_iter:d} - Loss: {tr[j, 0]:.2e} - Noise: {_softplus(tr[j, NP]) + NOISE_FLOOR:.2e}')
        self._d.update(gp_raw=raw, gp_raw_g=raw_g)
        gk = self.kernel if isinstance(self.kernel, GPKernel) else GPKernel(kern)
        rec = GPMultiTaskRecord(eng.to_host(raw), eng.to_host(raw_g), info_h[0], info_h[1], status, ard=gk.ard, scale=gk.scale)
        self.gpr_info_ = dict(kernel=self.kernel, n_train=m, iterations=int(info_h[0]), loss=float(info_h[1]), e=float(info_h[2]),
                              status=status.astype(np.int64), grad=info_h[4:4 + NP].copy(),
                              converged=bool(info_h[2] <= self.rel_error), lengthscale=rec.lengthscale.reshape(r, -1),
                              outputscale=rec.outputscale.copy(), task_noises=rec.task_noises.copy(), noise=rec.noise)
        self.Vr_sigma = np.ones((m, r)) * np.sqrt(rec.outputscale)
        self.models = [rec]
        self.likelihoods = [rec]

    def _update_mt(self, P_new, A_new, A_sigma_new, retrain, verbose, fixed_noise, append):
        """update() of a MultiTask object (the reference's branch, :657-663): the concatenated data replace the training set,
        then one evaluation at the kept values, or (``retrain``) the joint loop warm-started at the trained values with fresh
        Adam moments -- the learned task + shared noise on ALL points: the reference installs no fixed-noise likelihood here,
        so ``A_sigma_new`` is not required and only resizes ``Vr_sigma``."""
        for flag, name in ((fixed_noise, 'fixed_noise=True'), (append, 'append=True')):
            if flag:
                raise NotImplementedError(f"update({name}) is not built for gpr_type='MultiTask': its likelihood is the learned "
                                          'task + shared noise on every point.')
        if not hasattr(self, 'models'):
            raise AttributeError(f"'{type(self).__name__}' object has no attribute 'models'")
        eng = self._mt_engine()
        self.verbose = verbose
        kern, flags, r = self._gp_kernel()[0], self._mt_flags(), self._mt_r()
        P0_new = self._scale_params(P_new)
        A_new = np.asarray(A_new, dtype=np.float64)
        if A_new.ndim < 2:
            A_new = A_new[np.newaxis, :]
        if A_new.shape != (P0_new.shape[0], r):
            raise ValueError(f'A_new must have shape ({P0_new.shape[0]}, {r}), got {A_new.shape}.')
        P0_tot = np.concatenate([np.asarray(self.P0, dtype=np.float64), P0_new], axis=0)
        Vr_tot = np.concatenate([np.asarray(self.Vr, dtype=np.float64), A_new / np.asarray(self.Sigma_r)], axis=0)
        self._check_gp_inputs(P0_tot, Vr_tot, 'update')
        if A_sigma_new is not None:
            A_sigma_new = np.asarray(A_sigma_new, dtype=np.float64)
            if A_sigma_new.ndim < 2:
                A_sigma_new = A_sigma_new[np.newaxis, :]
            self.Vr_sigma = np.zeros((self.Vr_sigma.shape[0] + A_sigma_new.shape[0], r))
        self._mt_launch(eng, kern, flags, P0_tot, Vr_tot, self._d['gp_raw'], self._d['gp_raw_g'], bool(retrain), 'update')

    # ------------------------------------------------------------------ accumulating updates
    def _held_data(self, eng):
        """-> P0 (m, d), Y (m, r), w (m,), V (m, r) on the host: what the GPs are conditioned on now, with its noise"""
        P0, Y = eng.to_host(self._d['gp_P0']), eng.to_host(self._d['gp_Y'])
        m, r = Y.shape
        w = np.asarray(self.gpr_info_.get('noise_weight', np.ones(m)), dtype=np.float64)
        V = np.asarray(self.gpr_info_.get('fixed_noise', np.zeros((m, r))), dtype=np.float64)
        return P0, Y, w, V

    def _append_engine(self, gk, retrain=False):
        self._gp_engine(gk is not None)
        return self._engine_with(('gp_state', 'gp_append') + (('gp_train_noise',) if retrain else ()), 'gp.hip')

    def _append_state(self, eng, kern, flags, w, V, what):
        """-> X (r, m, m), logdet (r,) of the current K^-1; one gp_state launch where the object holds none that belongs to it
        (K^-1 and alpha then become that launch's)"""
        st = self.__dict__.get('_gp_state_of')
        if st is not None and st is self._d['gp_Kinv']:
            return self._gp_X, self._gp_logdet
        Kinv, alpha, info, X, logdet = eng.gp_state(self._d['gp_P0'], self._d['gp_Y'], eng.to_device(w), eng.to_device(V), kern, flags,
                                                    self._d['gp_raw'])
        self._raise_not_pd(eng.to_host(info)[:, 3], what)
        self._d.update(gp_Kinv=Kinv, gp_alpha=alpha)
        self._gp_X, self._gp_logdet, self._gp_state_of = X, logdet, Kinv      # (device tensors: never pickled)
        return X, logdet

    def _set_appended(self, m_tot, loss, w, V):
        r = len(self.models)
        self.gpr_info_.update(n_train=m_tot, loss=np.array(loss, dtype=np.float64), noise_weight=w, fixed_noise=V,
                              n_added=m_tot - np.shape(self.Vr)[0], grad=np.full_like(self.gpr_info_['grad'], np.nan))
        for i, rec in enumerate(self.models):
            rec.loss = float(loss[i])
        self.Vr_sigma = np.zeros((m_tot, r))

    def _update_append(self, P_new, A_new, A_sigma_new, retrain, verbose):
        """update(append=True): every refusal first, then at most one gp_state launch and one gp_append launch per 64 rows"""
        if retrain and A_sigma_new is None:
            raise NotImplementedError('update(retrain=True) trains with a fixed-noise likelihood: pass A_sigma_new (k, r), the '
                                      'standard deviations of A_new (the Ar_sigma / Ar_std of SPR.predict / assimilate); '
                                      'retrain=False keeps the hyper-parameters.')
        if not hasattr(self, 'models'):
            raise AttributeError(f"'{type(self).__name__}' object has no attribute 'models'")
        self.verbose = verbose
        kern, gk = self._gp_kernel()
        eng = self._append_engine(gk, retrain)
        r = len(self.models)
        Sigma_r = np.asarray(self.Sigma_r, dtype=np.float64)
        P0_new = self._scale_params(P_new)
        A_new = np.asarray(A_new, dtype=np.float64)
        if A_new.ndim < 2:
            A_new = A_new[np.newaxis, :]
        k = P0_new.shape[0]
        if k < 1 or A_new.shape != (k, r):
            raise ValueError(f'A_new must have shape ({k}, {r}) with at least one row, got {A_new.shape}.')
        Y_new = A_new / Sigma_r
        if not (np.all(np.isfinite(P0_new)) and np.all(np.isfinite(Y_new))):
            raise ValueError('update: the scaled P_new and A_new / Sigma_r must be finite.')
        if A_sigma_new is None:
            w_new, V_new = np.ones(k), np.zeros((k, r))
        else:
            A_sigma_new = np.asarray(A_sigma_new, dtype=np.float64)
            if A_sigma_new.ndim < 2:
                A_sigma_new = A_sigma_new[np.newaxis, :]
            if A_sigma_new.shape != (k, r):
                raise ValueError(f'A_sigma_new must have shape ({k}, {r}), got {A_sigma_new.shape}.')
            if not (np.all(np.isfinite(A_sigma_new)) and np.all(A_sigma_new >= 0)):
                raise ValueError('A_sigma_new must be finite and >= 0: it holds standard deviations.')
            w_new, V_new = np.zeros(k), (A_sigma_new / Sigma_r) ** 2
            if not np.all(np.isfinite(V_new)):
                raise ValueError('update: (A_sigma_new / Sigma_r)**2 has entries that are not finite.')
        m_cur = int(self.gpr_info_['n_train'])
        if m_cur + k > SPR_GP_MAX_M:
            raise NotImplementedError(f'update(append=True): {m_cur} held + {k} new points exceed the {SPR_GP_MAX_M} an exact '
                                      'Cholesky GP is built for; forget(keep_last=...) drops earlier measurements.')
        P0_cur, Y_cur, w_cur, V_cur = self._held_data(eng)
        P0_tot, Y_tot = np.concatenate([P0_cur, P0_new]), np.concatenate([Y_cur, Y_new])
        w, V = np.concatenate([w_cur, w_new]), np.concatenate([V_cur, V_new])
        if retrain:
            self._noise_launch(eng, kern, gk, P0_tot, Y_tot, w, V, True)
            self.gpr_info_['n_added'] = m_cur + k - np.shape(self.Vr)[0]
            return
        flags = 0 if gk is None else gk.flags
        X, logdet = self._append_state(eng, kern, flags, w_cur, V_cur, 'update')
        P0_d, Y_d, w_d, V_d = (eng.to_device(a) for a in (P0_tot, Y_tot, w, V))
        Kinv, alpha, raw, slices = self._d['gp_Kinv'], None, self._d['gp_raw'], []
        for m_end in list(range(m_cur + SPR_GP_MAX_APPEND, m_cur + k, SPR_GP_MAX_APPEND)) + [m_cur + k]:
            rows = m_end - Kinv.shape[1]
            X, Kinv, alpha, logdet, info = eng.gp_append(P0_d[:m_end], Y_d[:m_end], w_d[:m_end], V_d[:m_end], kern, flags, raw, X,
                                                         Kinv, logdet, rows)
            info_h = eng.to_host(info)
            slices.append(dict(rows=rows, status=info_h[:, 3].astype(np.int64), logdet=info_h[:, 2].copy()))
            self._raise_not_pd(info_h[:, 3], 'update')            # nothing of this call is kept
        self._d.update(gp_P0=P0_d, gp_Y=Y_d, gp_Kinv=Kinv, gp_alpha=alpha)
        self._gp_X, self._gp_logdet, self._gp_state_of = X, logdet, Kinv
        self.append_info_ = slices
        self._set_appended(m_cur + k, info_h[:, 1], w, V)

    def forget(self, keep_last=0):
        """Drop the points that updates added, except the last ``keep_last`` of them: the GPs are conditioned on the
        simulations of fit() and those points, at the kept hyper-parameters, and the state of ``update(append=True)`` is
        established again by one factorisation (``engine.gp_state``, O(m^3)) -- rows are not removed from a factor one by one.
        This is how a long-running loop stays under 800 points."""
        if self.gpr_type == 'MultiTask':
            raise NotImplementedError("forget is not built for gpr_type='MultiTask': its updates do not accumulate (append=True "
                                      'is not built either).')
        if not hasattr(self, 'models'):
            raise AttributeError(f"'{type(self).__name__}' object has no attribute 'models'")
        if not (isinstance(keep_last, (int, np.integer)) and keep_last >= 0):
            raise ValueError(f'forget: keep_last must be a non-negative int, got {keep_last!r}')
        kern, gk = self._gp_kernel()
        eng = self._append_engine(gk)
        P0, Y, w, V = self._held_data(eng)
        m_fit, m_cur = np.shape(self.Vr)[0], len(P0)
        keep = np.r_[0:m_fit, max(m_fit, m_cur - int(keep_last)):m_cur]
        P0, Y, w, V = P0[keep], Y[keep], w[keep], V[keep]
        flags = 0 if gk is None else gk.flags
        P0_d, Y_d = eng.to_device(P0), eng.to_device(Y)
        Kinv, alpha, info, X, logdet = eng.gp_state(P0_d, Y_d, eng.to_device(w), eng.to_device(V), kern, flags, self._d['gp_raw'])
        info_h = eng.to_host(info)
        self._raise_not_pd(info_h[:, 3], 'forget')
        self._d.update(gp_P0=P0_d, gp_Y=Y_d, gp_Kinv=Kinv, gp_alpha=alpha)
        self._gp_X, self._gp_logdet, self._gp_state_of = X, logdet, Kinv
        self._set_appended(len(keep), info_h[:, 1], w, V)
