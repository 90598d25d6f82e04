"""Host algebra of ROM.partial_fit: one step of the block incremental SVD (Brand 2002 / 2006; the rank-k update behind
scikit-learn's IncrementalPCA) on plain ndarrays, float64, small matrices only.

The device passes around it (csrc/update.hip, csrc/validate.hip) hand over, for a batch X0_b (n, k) in the scaled units of
fit() and the held orthonormal basis U (n, r):

    C  = X0_b^T U                 (k, r)   spr_encode_*
    H  = E^T E,  C2 = E^T U,  ss = sum X0_b^2      with E = X0_b - U C^T        spr_subspace_residual_*

and take back the two small matrices of  U_new = U A + X0_b B  (spr_basis_update_*).

Why C2: in exact arithmetic E^T U = 0.  The held U is orthonormal to rounding only, and every update
U A + X0_b B cancels -- it loses about eps / (relative residual) of orthogonality.  Left alone that defect re-enters the next
residual as spurious directions above ``tol`` (ten batches of 16 at tol = 1e-7: max |U^T U - I| = 3.6e-3 without the
correction, 2.5e-10 with it).  C2 is the second pass of classical Gram-Schmidt done in the small matrices:
E_c = E - U C2^T = X0_b - U (C + C2)^T, and E_c^T E_c = H - C2 C2^T up to terms of the order of the defect squared.
"""
from __future__ import annotations

import numpy as np

MAX_RANK = 128        # SPR_MAX_R: the width the update kernels are built for
MAX_BATCH = 64        # columns of one update


def initial_energy(S, exp_variance):
    """Energy of everything fit() saw, from what it leaves: sum(S_r^2) * 100 / exp_variance_[r - 1]."""
    S = np.asarray(S, dtype=np.float64)
    return float(np.sum(S ** 2) * 100.0 / float(exp_variance[len(S) - 1]))


def select_rank(sig2, E_tot, r, q, select_modes, n_modes):
    """r' after an update whose small SVD has r + q singular values (squares ``sig2``, descending)"""
    top = r + q
    if select_modes is None:
        r2 = min(r, top)
    elif select_modes == 'number':
        if type(n_modes) is not int:
            raise TypeError('The parameter n_modes is not an integer.')
        if n_modes < 1:
            raise ValueError('The parameter n_modes is below 1.')
        r2 = min(n_modes, top)
    elif select_modes == 'variance':
        if not 0 <= n_modes <= 100:
            raise ValueError('The parameter n_modes is outside the[0-100] range.')
        ev = 100.0 * np.cumsum(sig2) / E_tot
        hit = np.nonzero(ev >= n_modes)[0]
        r2 = int(hit[0]) + 1 if hit.size else top
    else:
        raise ValueError('The select_mode value is wrong.')
    return r2


def svd_update(S, Ar, C, H, C2, ss, E_tot, *, tol=1e-7, select_modes=None, n_modes=None, max_rank=MAX_RANK, correct=True):
    """One update.  S (r,), Ar (m, r) = V diag(S), C / C2 (k, r), H (k, k), ss and E_tot scalars.

    -> dict: A (r, r'), B (k, r'), S (r',), Ar (m + k, r'), E_tot, exp_variance (r',), q, dropped, residual, orth_defect.
    Raises ValueError for a non-finite batch (seen in ss / H) and NotImplementedError for r' > max_rank; nothing of the
    caller's is modified in either case.  ``correct=False`` leaves the C2 correction out (tests: it is required)."""
    S = np.asarray(S, dtype=np.float64)
    Ar = np.asarray(Ar, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    H = np.asarray(H, dtype=np.float64)
    C2 = np.asarray(C2, dtype=np.float64)
    ss = float(np.asarray(ss).reshape(-1)[0])
    r, k = S.shape[0], C.shape[0]
    if not (np.isfinite(ss) and np.all(np.isfinite(H)) and np.all(np.isfinite(C)) and np.all(np.isfinite(C2))):
        raise ValueError('X_new holds values that are not finite.')
    if correct:
        Ct = C + C2
        Hc = H - C2 @ C2.T
    else:
        Ct = C
        Hc = H
    Hc = 0.5 * (Hc + Hc.T)
    lam, W = np.linalg.eigh(Hc)
    lam, W = lam[::-1], W[:, ::-1]
    lam0 = max(float(lam[0]), 0.0)
    thr = (tol * max(float(S[0]), np.sqrt(lam0))) ** 2
    q = int(np.count_nonzero(lam > thr))
    T = W[:, :q] / np.sqrt(lam[:q])                          # (k, q): E_c T has orthonormal columns
    R = T.T @ Hc                                             # (q, k)
    K = np.zeros((r + q, r + k))
    K[:r, :r] = np.diag(S)
    K[:r, r:] = Ct.T
    K[r:, r:] = R
    P, sig, Wt = np.linalg.svd(K, full_matrices=False)
    E_new = float(E_tot) + ss
    r2 = select_rank(sig ** 2, E_new, r, q, select_modes, n_modes)
    if r2 > max_rank:
        raise NotImplementedError(f'partial_fit would keep {r2} modes; the update kernels are built for at most {max_rank}.')
    P1, P2 = P[:r, :r2], P[r:, :r2]
    B = T @ P2
    A = P1 - Ct.T @ B
    with np.errstate(divide='ignore', invalid='ignore'):
        V = np.where(S > 0, Ar / S, 0.0)
    m = Ar.shape[0]
    Wk = Wt.T[:, :r2]                                        # (r + k, r')
    Ar_new = np.vstack([V @ Wk[:r], Wk[r:]]) * sig[:r2]
    assert Ar_new.shape == (m + k, r2)
    trH, trHc = float(np.trace(H)), float(np.trace(Hc))
    return dict(A=np.ascontiguousarray(A), B=np.ascontiguousarray(B), S=sig[:r2].copy(), Ar=Ar_new, E_tot=E_new,
                exp_variance=100.0 * np.cumsum(sig[:r2] ** 2) / E_new, q=q,
                dropped=float(np.sum(np.maximum(lam[q:], 0.0)) + np.sum(sig[r2:] ** 2)),
                residual=float(np.sqrt(max(trHc, 0.0) / ss)) if ss > 0 else 0.0,
                orth_defect=float(np.linalg.norm(C2) / np.sqrt(trH)) if trH > 0 else 0.0)
