"""predict() for train(method='COLS'): the reference's constrained least squares (sparse_sensing.py:880-892)

    minimise   || W (y0 - Theta g) ||^2        subject to   lo0 <= Ur g <= hi0      (2 n rows)

by CONSTRAINT GENERATION.  The unknown has r entries and almost none of the 2 n constraints bind, so the quadratic
programme is only ever solved on a small working set of rows:

    round 0   g = the unconstrained (OLS) solution of the existing solve path
    sweep     one streaming pass over the basis (engine.bound_sweep, csrc/bounds.hip): worst violation, number of
              violated rows, and the worst row per side of every workgroup's run of rows as candidates
    done?     max violation <= cols_tol  ->  g is feasible for ALL rows, and optimal on a subset of them: optimal
    grow      add the cols_rows_per_round worst candidates (rows are only ever added), fetch their rows of Ur and
              X_cnt with measure_csr, solve the working-set QP exactly on the host in f64, sweep again

Rows are only ever added, so the loop ends after finitely many rounds, and the multipliers of the last QP (zero on
every row outside the working set) are a KKT certificate for the full problem.  H = Theta^T W^2 Theta is positive
definite (rank-deficient W Theta is refused), so that point is THE solution.

The working-set QP  min 1/2 g^T H g - f^T g,  A g <= b  becomes a least-distance problem  min |z|^2, M z <= d  with
H = L L^T, z = L^T (g - g_ols), M = A L^-T, d = b - A g_ols, solved through NNLS (Lawson & Hanson, ch. 23); the active
set NNLS finds is then re-solved as an equality-constrained problem (one small Cholesky), which removes the
1 / (1 + |z|^2) scaling error of the least-distance form.  Same division of labour as the m x m eigen-problem
(_eigen.py): the n-sized work is on the device, the working-set-sized work on the host.

Sharded objects: every rank sweeps its block; the ranks' result records are all-gathered and merged by the rule the
kernel uses (worst first, ties to the lower global row, then the lower side), so all ranks solve the identical QP.
Per round: one all-gather (sweep records) and, when rows are added, two all-reduces (the rows of Ur, X_cnt).
"""
import time

import numpy as np

#: ||rho|| of the NNLS residual below which the working set is declared infeasible: |rho|^2 = 1 / (1 + |z|^2), so
#: this is a solution more than 1e7 (scaled, whitened) units away from the unconstrained one
_INFEASIBLE_RHO = 1e-7


def feature_clamps(limits, cnt_minmax, scl_f):
    """(2, F) array: NaN, or the constant the reference substitutes for the scaled limit of a whole feature block
    (:201-204: -1000 when the smallest scaled limit is below -1000, else +1000 when the largest is above 1000).
    (limit - X_cnt) / X_scl is monotone in X_cnt, so the extremes come from the per-feature min / max of X_cnt."""
    F = len(scl_f)
    out = np.full((2, F), np.nan)
    for j, limit in enumerate(limits):
        for f in range(F):
            t = (limit[f] - cnt_minmax[f]) / scl_f[f]
            if t.min() < -1000:
                out[j, f] = -1000
            elif t.max() > 1000:
                out[j, f] = 1000
    return out


def solve_working_qp(L, g_ols, A, b):
    """min 1/2 g^T H g - f^T g  s.t.  A g <= b,  H = L L^T, g_ols = H^-1 f.
    -> (g, multipliers >= 0) or (None, None) when the rows are infeasible."""
    from scipy.linalg import solve_triangular
    from scipy.optimize import nnls
    r = L.shape[0]
    M = solve_triangular(L, A.T, lower=True).T               # A L^-T
    d = b - A @ g_ols
    nrm = np.sqrt(np.sum(M * M, axis=1))
    nrm[nrm == 0] = 1.0
    Mn, dn = M / nrm[:, None], d / nrm
    # least distance  min |z|, G z >= h  with G = -Mn, h = -dn:  E = [G^T; h^T], f = e_{r+1}
    E = np.vstack([-Mn.T, -dn[None, :]])
    rhs = np.zeros(r + 1)
    rhs[r] = 1.0
    u, _ = nnls(E, rhs, maxiter=max(30 * E.shape[1], 300))
    rho = E @ u - rhs
    if np.linalg.norm(rho) < _INFEASIBLE_RHO or not rho[r] < 0:
        return None, None
    lam = u / (-rho[r]) / nrm
    act = np.flatnonzero(u > 0)
    g = g_ols - solve_triangular(L, M.T @ lam, lower=True, trans='T')
    if len(act):
        # polish: the active rows as equalities,  S lam_a = A_a g_ols - b_a,  S = M_a M_a^T
        Ma = M[act]
        try:
            S = Ma @ Ma.T
            c = np.linalg.cholesky(S)
            la = solve_triangular(c, solve_triangular(c, -d[act], lower=True), lower=True, trans='T')
            gp = g_ols - solve_triangular(L, Ma.T @ la, lower=True, trans='T')
            worst = lambda x: float(np.max(A @ x - b))            # noqa: E731
            if np.all(la >= 0) and worst(gp) <= max(worst(g), 0.0) + 1e-12:
                lam = np.zeros(len(b))
                lam[act] = la
                g = gp
        except np.linalg.LinAlgError:
            pass                                                  # dependent active rows: keep the NNLS point
    return g, lam


def merge_records(rec, k):
    """rec (world, n_p, 3 + 3 k') sweep records of the ranks -> per vector (max violation, its row, count,
    [(row, side, v), ...] worst first, ties to the lower row, then the lower side, at most k)."""
    world, n_p, w = rec.shape
    out = []
    for p in range(n_p):
        best_v, best_row, count = -np.inf, -1, 0
        cands = []
        for q in range(world):
            v, row, cnt = rec[q, p, 0], int(rec[q, p, 1]), int(rec[q, p, 2])
            if row >= 0 and (v > best_v or (v == best_v and row < best_row)):
                best_v, best_row = float(v), row
            count += cnt
            c = rec[q, p, 3:].reshape(-1, 3)
            cands += [(int(a), int(s), float(x)) for a, s, x in c if a >= 0]
        cands.sort(key=lambda t: (-t[2], t[0], t[1]))
        out.append((best_v, best_row, count, cands[:k]))
    return out


def generate_constraints(obj, G, lim, clamp, tol, per_round, max_rounds, max_rows, solve, sweep, labels):
    """The constraint-generation loop of predict_cols and _cpod.constrain_pod on the fitted block of ``obj``: sweep, merge
    the ranks' records, grow the working sets of the vectors that still violate, solve their QPs, until none is active.

    ``G`` (n_p, r): the unconstrained solutions, overwritten row by row;  ``lim`` / ``clamp`` (2, F): the limits and
    feature_clamps of them;  ``solve(p, A, b) -> (g | None, multipliers)``: vector p's working-set QP;
    ``sweep(n_active) -> engine method``: the bound sweep for that many active vectors;  ``labels`` = (name, item, knob
    prefix) of the messages, e.g. ('COLS', 'vector', 'cols').
    -> (G, info): info = dict(vectors = the per-vector dicts, sweeps, sweep_seconds, rows_seconds, qp_seconds, cached_rows)
    and the per-vector entries again as one list per key; the callers publish what is theirs of it."""
    name, item, knob = labels
    eng = obj._engine()
    F, n_points, scl_f = obj.n_features, obj.n_points, obj._scl_f
    lim_d, clamp_d = eng.to_device(lim), eng.to_device(clamp)
    blk = obj._block()
    n_p, r = G.shape
    info = [dict(status=None, rounds=0, rows=np.zeros(0, dtype=np.int64), sides=np.zeros(0, dtype=np.int64),
                 multipliers=np.zeros(0), max_violation=np.nan, violated=0) for _ in range(n_p)]
    work = [dict(keys={}, A=np.zeros((0, r)), b=np.zeros(0)) for _ in range(n_p)]
    active = list(range(n_p))
    sweeps, t_sweep, t_qp, t_rows = 0, 0.0, 0.0, 0.0
    rows_cache = {}                                                           # global row -> (u, X_cnt), all vectors
    while active:
        t0 = time.perf_counter()
        rec_d = sweep(len(active))(*blk, lim_d, clamp_d, eng.to_device(G[active]), tol, per_round)
        rec = eng.to_host(obj._all_gather(rec_d))
        t_sweep += time.perf_counter() - t0
        sweeps += 1
        merged = merge_records(rec, per_round)
        grow = []
        for p, (v, row, count, cands) in zip(active, merged):
            info[p]['rounds'] += 1
            info[p]['max_violation'], info[p]['violated'] = v, count
            if not np.all(np.isfinite(G[p])):
                raise np.linalg.LinAlgError(f'{name}: {item} {p} has non-finite coefficients')
            if v <= tol:
                info[p]['status'] = 'ols' if info[p]['rounds'] == 1 else 'optimal'
                continue
            if info[p]['rounds'] >= max_rounds:
                raise RuntimeError(f'{name}: {item} {p} still violates its limits by {v:.3e} (tolerance {tol:.1e}, {count} '
                                   f'rows) after {knob}_max_rounds = {max_rounds} sweeps')
            new = [c for c in cands if (c[0], c[1]) not in work[p]['keys']]
            if not new:
                raise RuntimeError(f'{name}: {item} {p} violates row {row} by {v:.3e} although the row is in the working '
                                   f'set: {knob}_tol = {tol:.1e} is below what the working-set solve resolves')
            if len(work[p]['keys']) + len(new) > max_rows:
                raise RuntimeError(f'{name}: {item} {p} needs more than {knob}_max_rows = {max_rows} working rows')
            grow.append((p, new))
        active = [p for p, _ in grow]
        if not grow:
            break
        # rows of Ur (and X_cnt) of the new candidates: one-hot CSR through measure_csr, as train() builds Theta
        t0 = time.perf_counter()
        need = sorted({c[0] for _, new in grow for c in new} - set(rows_cache))
        if need:
            idx = np.asarray(need, dtype=np.int64)
            t = eng.torch
            ip, ix, vv = (eng.to_device(np.arange(len(idx) + 1), dtype=t.int64), eng.to_device(idx, dtype=t.int64),
                          eng.to_device(np.ones(len(idx))))
            U_d, c_d = eng.measure_csr(ip, ix, vv, blk.Ur, blk.row0, blk.rowmean)
            U_h, c_h = eng.to_host(obj._all_reduce(U_d)), eng.to_host(obj._all_reduce(c_d))
            for i, row in enumerate(need):
                rows_cache[row] = (np.array(U_h[i], dtype=np.float64), float(c_h[i]))
        t_rows += time.perf_counter() - t0
        t0 = time.perf_counter()
        for p, new in grow:
            wk = work[p]
            A_new, b_new = np.empty((len(new), r)), np.empty(len(new))
            for i, (row, side, _) in enumerate(new):
                u, cnt = rows_cache[row]
                f = min(row // n_points, F - 1)
                lim0 = clamp[side, f] if not np.isnan(clamp[side, f]) else (lim[side, f] - cnt) / scl_f[f]
                A_new[i], b_new[i] = (u, lim0) if side == 1 else (-u, -lim0)     # u g <= hi0  |  -u g <= -lo0
                wk['keys'][(row, side)] = len(wk['keys'])
            wk['A'], wk['b'] = np.vstack([wk['A'], A_new]), np.concatenate([wk['b'], b_new])
            g, lam = solve(p, wk['A'], wk['b'])
            keys = sorted(wk['keys'], key=wk['keys'].get)
            info[p]['rows'] = np.asarray([k[0] for k in keys], dtype=np.int64)
            info[p]['sides'] = np.asarray([k[1] for k in keys], dtype=np.int64)
            if g is None:
                info[p]['status'] = 'infeasible'
                info[p]['multipliers'] = np.full(len(keys), np.nan)
                G[p] = np.nan                           # the reference's Ar[i, :] = None (:892); its Gr[:, i] stays unset
                active.remove(p)
            else:
                G[p], info[p]['multipliers'] = g, lam
        t_qp += time.perf_counter() - t0
    raw = dict(vectors=info, sweeps=sweeps, sweep_seconds=t_sweep, rows_seconds=t_rows, qp_seconds=t_qp,
               cached_rows=len(rows_cache))
    for key in ('status', 'rounds', 'rows', 'sides', 'multipliers', 'max_violation'):
        raw[key] = [v[key] for v in info]
    return G, raw


def predict_cols(spr, ys):
    """(Ar, Ar_sigma) of SPR.predict for method == 'COLS'; leaves spr.cols_info_."""
    eng = spr._engine()
    F = spr.n_features
    limits = [np.asarray(limit, dtype=np.float64) for limit in spr.limits]   # None: the reference's TypeError (:883)
    if len(limits) != 2 or any(l.ndim != 1 or l.shape[0] < F for l in limits):
        raise ValueError('limits has to be a list of two arrays with n_features entries (minimum, maximum).')
    Theta = spr.Theta
    s, r = Theta.shape
    if s < r:
        raise NotImplementedError(f"method='COLS' with fewer sensors ({s}) than modes ({r}): the minimiser is not unique and "
                                  'the reference returns whatever its solver stops at; not part of this implementation.')
    Ar, Ar_sigma, y0 = spr._solve(ys)
    if getattr(spr, 'solve_path_', None) != 'cholesky':
        raise NotImplementedError("method='COLS' with a rank-deficient (or numerically rank-deficient) W Theta: the minimiser "
                                  'is not unique and the reference returns whatever its solver stops at; not part of this '
                                  'implementation.')
    n_p = len(ys)
    tol, per_round = float(spr.cols_tol), int(spr.cols_rows_per_round)
    max_rounds, max_rows = int(spr.cols_max_rounds), int(spr.cols_max_rows)
    if not (tol >= 0 and 0 < per_round <= 256 and max_rounds > 0):
        raise ValueError('cols_tol must not be negative, cols_rows_per_round must be in 1..256, cols_max_rounds positive')

    lim = np.stack([l[:F] for l in limits])                                   # (2, F)
    clamp = feature_clamps(lim, spr._cols_cnt_minmax, spr._scl_f)

    # per vector: H = Theta^T W^2 Theta = L L^T (W as in the OLS branch, :866-874)
    Ls = []
    for p in range(n_p):
        w = 1.0 / y0[p, :, 1] if np.any(np.asarray(ys[p])[:, 1]) else np.ones(s)
        WT = Theta * w[:, None]
        try:
            Ls.append(np.linalg.cholesky(WT.T @ WT))
        except np.linalg.LinAlgError:
            raise NotImplementedError("method='COLS' with a rank-deficient W Theta: the minimiser is not unique; not part of "
                                      'this implementation.') from None

    G, raw = generate_constraints(spr, Ar.copy(), lim, clamp, tol, per_round, max_rounds, max_rows,
                                  solve=lambda p, A, b: solve_working_qp(Ls[p], Ar[p], A, b),
                                  sweep=lambda n_active: eng.bound_sweep, labels=('COLS', 'vector', 'cols'))
    spr.cols_info_ = {key: v for key, v in raw.items() if key not in ('rows_seconds', 'cached_rows')}
    return G, Ar_sigma
