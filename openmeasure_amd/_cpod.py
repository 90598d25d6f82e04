"""ROM.CPOD: the reference's constrained POD (sparse_sensing.py:434-461) for the problem its documentation solves, once per
snapshot i,

    minimise   || Ur g - X0[:, i] ||_2        subject to   lo0 <= Ur g <= hi0,      (lo0, hi0) = scale_limits([lo, hi])

by the CONSTRAINT GENERATION of _cols.py.  Ur^T Ur = I for a basis fit() computed, so the objective is
|g - a_i|^2 + const with a_i = Ur^T X0[:, i] = the row of Ar fit() already holds: X0 is never formed, the unconstrained
optimum needs no solve and the working-set QP has H = I.  The loop is predict_cols' with L = I, g_ols = Ar0[i] and
vectors = snapshots:

    sweep     one pass over the basis for all still-active snapshots (engine.bound_sweep_batch, csrc/bounds.hip: 64 vectors
              per read of the basis; fewer than BATCH_FROM = 33 vectors, or an engine without it, take engine.bound_sweep)
    done?     max violation <= cpod_tol: feasible for ALL rows and optimal on a subset of them: optimal
    grow      add the cpod_rows_per_round worst candidates, fetch their rows of Ur and X_cnt through measure_csr (one cache
              for all snapshots: neighbouring snapshots violate the same cells), solve the working-set QP, sweep again

The working-set QP is a least-distance problem  min |z|, A z <= d  (z = g - a, d = b - A a).  Unlike COLS, whose solutions
stay near the unconstrained one, a snapshot can end far from its OLS coefficients (|z| of 10 ... 100 scaled units against
|d| of 1e-3) with nearly parallel rows in the set -- neighbouring cells.  _cols.solve_working_qp returns points that
violate their own rows by 1e-4 ... 1e-2 there, for two reasons: the residual of its NNLS form carries a factor
1 / (1 + |z|^2), and SciPy's nnls stops at points that miss their own optimality conditions by 1e-2 on such columns
(measured: gradient on the positive set 9e-3 ... 1e-1).  solve_distance_qp therefore solves for z / t with t an estimate
of |z| (so the scaled solution has length about one) with an NNLS written out here (_nnls: Lawson & Hanson with SVD
least-squares solves), re-solves with t = |z| of the previous attempt while rows of the set are still violated, and
finishes with the active rows as equalities.

Sharded objects as in _cols.py: every rank sweeps its block, one all-gather of records per round, all-reduced rows from
measure_csr, every rank solves the identical QPs.
"""
import numpy as np

from ._cols import _INFEASIBLE_RHO, feature_clamps, generate_constraints

#: fewer active snapshots than this are swept with engine.bound_sweep (16 vectors per pass): the batched kernel pays for
#: 64 vectors per pass whatever their number.  Measured at 90M rows x r = 64, 16-vector kernel
#: against batched: 16 vectors 7.9 / 12.0 ms, 32 vectors 15.6 / 15.1 (a draw: 1.03 x; 1.13 x at 4M rows x r = 32),
#: 48 vectors 23.3 / 17.9 (1.31 x), 64 vectors 31.1 / 21.7.  Both kernels work in groups of 16 vectors, so 17 ... 32 cost
#: what 32 do: the switch sits above the draw, at the first count where the batched kernel clearly wins
BATCH_FROM = 33

#: solve_distance_qp: a returned point may violate a row of its own working set by this much (scaled units, relative to
#: 1 + |b_i|); the attempts stop there.  Two orders below the default cpod_tol.
_ROW_TOL = 1e-11
_MAX_ATTEMPTS = 6


def _nnls(E, f):
    """min |E x - f|, x >= 0: Lawson & Hanson's active-set algorithm (ch. 23) with every passive-set solve done by an
    SVD least squares, so nearly parallel columns -- rows of neighbouring cells -- cost accuracy nowhere.  Written out
    here because the result has to satisfy its own optimality conditions to rounding: the multipliers of the QP are read
    from it."""
    n = E.shape[1]
    P = np.zeros(n, dtype=bool)
    x = np.zeros(n)
    tol = 10 * np.finfo(np.float64).eps * max(np.abs(E).sum(axis=0).max(), 1.0) * max(np.abs(f).max(), 1.0)
    banned = np.zeros(n, dtype=bool)
    for _ in range(3 * n + 30):
        w = E.T @ (f - E @ x)
        w[P | banned] = -np.inf
        j = int(np.argmax(w))
        if not w[j] > tol:
            break
        P[j] = True
        s = np.zeros(n)
        s[P] = np.linalg.lstsq(E[:, P], f, rcond=None)[0]
        if not s[j] > 0:                                   # rounding: the column cannot enter although its gradient says so
            P[j], banned[j] = False, True
            continue
        for _ in range(3 * n + 30):
            neg = P & (s <= 0)
            if not neg.any():
                break
            alpha = np.min(x[neg] / (x[neg] - s[neg]))
            x = x + alpha * (s - x)
            P &= ~(neg & (x <= tol)) & (x > 0)
            x[~P] = 0.0
            s = np.zeros(n)
            if P.any():
                s[P] = np.linalg.lstsq(E[:, P], f, rcond=None)[0]
        x = s
        banned[:] = False
    return x


def _ldp(A, d):
    """min |z|^2, A z <= d through NNLS (Lawson & Hanson ch. 23) -> (z, multipliers u with z = -A^T u) or None."""
    r = A.shape[1]
    E = np.vstack([-A.T, -d[None, :]])
    rhs = np.zeros(r + 1)
    rhs[r] = 1.0
    u = _nnls(E, rhs)
    rho = E @ u - rhs
    if np.linalg.norm(rho) < _INFEASIBLE_RHO or not rho[r] < 0:
        return None
    lam = u / (-rho[r])
    return -A.T @ lam, lam


def _polish(A, d, act):
    """the rows `act` as equalities: min |z|^2, A_a z = d_a -> (z, multipliers) or None (dependent rows, negative sign)"""
    from scipy.linalg import solve_triangular
    Aa = A[act]
    try:
        c = np.linalg.cholesky(Aa @ Aa.T)
    except np.linalg.LinAlgError:
        return None
    la = solve_triangular(c, solve_triangular(c, -d[act], lower=True), lower=True, trans='T')
    if not np.all(la >= 0):
        return None
    return -Aa.T @ la, la


def solve_distance_qp(a, A, b):
    """min 1/2 |g - a|^2  s.t.  A g <= b  (the working-set QP of CPOD: H = I).
    -> (g, multipliers >= 0 with g - a + A^T lambda = 0) or (None, None) when the rows are infeasible."""
    nrm = np.sqrt(np.sum(A * A, axis=1))
    nrm[nrm == 0] = 1.0
    An, dn = A / nrm[:, None], (b - A @ a) / nrm
    bn = np.abs(b) / nrm
    if dn.min() >= 0:
        return a.copy(), np.zeros(len(b))
    t = -dn.min()                                  # the worst row alone is this far away: a lower bound of |z|
    best = None
    for _ in range(_MAX_ATTEMPTS):
        got = _ldp(An, dn / t)
        if got is None:
            if best is None:
                return None, None
            break
        z, lam = got[0] * t, got[1] * t
        act = np.flatnonzero(lam > 0)
        pol = _polish(An, dn, act) if len(act) else None
        worst = float(np.max((An @ z - dn) / (1.0 + bn)))
        if pol is not None:
            wp = float(np.max((An @ pol[0] - dn) / (1.0 + bn)))
            if wp <= max(worst, _ROW_TOL):
                z, worst = pol[0], wp
                lam = np.zeros(len(b))
                lam[act] = pol[1]
        if best is None or worst < best[0]:
            best = (worst, z, lam)
        if worst <= _ROW_TOL:
            break
        t_new = float(np.linalg.norm(z))
        if not t_new > 0 or abs(t_new - t) <= 1e-3 * t:
            break
        t = t_new
    _, z, lam = best
    return a + z, lam / nrm


def constrain_pod(rom, limits, Ar0):
    """-> Gr (m, r): row i solves snapshot i's problem (NaN where the limits are infeasible); leaves rom.cpod_info_."""
    eng = rom._engine()
    F = rom.n_features
    limits = [np.asarray(limit, dtype=np.float64) for limit in limits]
    if len(limits) != 2 or any(l.ndim != 1 or l.shape[0] < F for l in limits):
        raise ValueError('limits has to be a list of two arrays with n_features entries (minimum, maximum).')
    tol, per_round = float(rom.cpod_tol), int(rom.cpod_rows_per_round)
    max_rounds, max_rows = int(rom.cpod_max_rounds), int(rom.cpod_max_rows)
    if not (tol >= 0 and 0 < per_round <= 256 and max_rounds > 0):
        raise ValueError('cpod_tol must not be negative, cpod_rows_per_round must be in 1..256, cpod_max_rounds positive')

    lim = np.stack([l[:F] for l in limits])                                   # (2, F)
    clamp = feature_clamps(lim, rom._feature_cnt_minmax(), rom._scl_f)
    batch = getattr(eng, 'bound_sweep_batch', None)
    G, rom.cpod_info_ = generate_constraints(
        rom, Ar0.copy(), lim, clamp, tol, per_round, max_rounds, max_rows,
        solve=lambda p, A, b: solve_distance_qp(Ar0[p], A, b),
        sweep=lambda n_active: batch if batch is not None and n_active >= BATCH_FROM else eng.bound_sweep,
        labels=('CPOD', 'snapshot', 'cpod'))
    return G
