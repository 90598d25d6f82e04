"""The core of the placement (csrc/qr_pivot.hip: the init and refresh sweeps qr_refresh_{direct,mfma,wide}_kernel,
qr_tops_from_norms_kernel, the candidate build, qr_orth_kernel / qr_step_fused_kernel / the three-launch step) on the CPU:
the case tables, the bases and the long-double references that tests/test_pivot_kernels_gpu.py holds the kernels'
intermediate quantities against -- squared row norms, the bound tau, the record, the certification flags, the directions --
and the checks of those references themselves: against LAPACK's pivot order, against the float64 NumPy double of the engine,
and that every case has the property it was built for (decisive gaps, decisive certification, residuals that stay a tenth of
their rows, a planted basis whose second pivot is a non-candidate).

Error bars (u = 2^-53, |u_i|^2 the long-double norm of the stored row), derived, not tuned:
  init     |nrm_i - ref| <= (r + 2) u |u_i|^2                 r non-negative rounded products summed in any order
  refresh  |nrm_i - ref| <= 2 ((2 r + 1) sqrt(nq) + nq + 2) u |u_i|^2
           a dot product errs by r u |u_i| |q|, its square by (2 r + 1) u |d_j| |u_i|, sum_j |d_j| <= sqrt(nq) |u_i| for
           orthonormal directions, the nq additions and the subtraction add (nq + 1) u |u_i|^2; the factor 2 covers
           |q| <= 1 + r u and fused against unfused products
  gap      (best - second) / best from the record's own values: 4 u relative
  Q        no closed bound for two-pass Gram-Schmidt: the float64 double (NumpyEngine.qr_step) is measured against the
           long-double reference on the step cases (twin_direction_errors); a device may err 8 times the double's worst
           value over the case list, plus r u."""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import spr_oracle as orc
from tests.numpy_engine import NumpyEngine

# rows of a sweep panel and rows a workgroup keeps: csrc/qr_pivot.hip, `rows_it` of sweep_grid (R of the sweep kernels) and QR_TOPT
PANEL, TOPT = 64, 16
MAX_BLOCKS = 1024                                 # QR_MAX_BLOCKS: cap of the sweep grid
QR_BATCH = 16                                     # spr_qr_batch() (the GPU file asserts it)
MAX_R = 128                                       # SPR_MAX_R: fused steps up to here, three launches above
GROUP = 16                                        # columns of an MFMA tile: what launch_refresh's kernel choice counts in
LD = np.longdouble
U_RND = 2.0 ** -53
DECISIVE = 1e-6


# ---- tables ---------------------------------------------------------------------------------------------------------------
ROWS = (1, 15, 16, 17, 63, 64, 65, 200, 323)      # 323 = 5 panels + 3 rows
N_TABLE = 323
N_STRIDE = 65536 + 69                             # more panels than MAX_BLOCKS: workgroups 0 and 1 take a second panel
STRIDE_CASES = ((16, 'contig'), (16, 'f32'), (144, 'contig'))
# beyond the widths that reach every family's first member -- 18, 34: pair loads with a column tail at MTR 2 and 3; 112: direct NG 7
NARROW_R = (1, 2, 3, 5, 16, 17, 18, 31, 32, 33, 34, 48, 50, 64, 80, 96, 100, 112, 128)
WIDE_R = (129, 144, 256, 272, 512, 528, 1024)
ALL_R = NARROW_R + WIDE_R
ROWS_R = (5, 16, 50, 144)                         # the widths every row count meets
ROW0S = (0, 1000)
# name -> (storage type, ldu - r, elements between the (aligned) buffer and the view)
LAYOUTS = {'contig': (np.float64, 0, 0), 'ld+1': (np.float64, 1, 0), 'ld+2': (np.float64, 2, 0),
           'off1': (np.float64, 2, 1), 'f32': (np.float32, 0, 0), 'f32-ld+4': (np.float32, 4, 0)}
SLACK = 8                                         # NaNs behind the last row


def round_mt(r):
    return next(s for s in (1, 2, 3, 4, 6, 8) if s >= -(-r // GROUP))


def sweep_family(r, layout, init):
    """The kernel launch_refresh selects (its rules restated) -- for the case ids and the coverage list."""
    dt, pad, off = LAYOUTS[layout]
    size, ldu = np.dtype(dt).itemsize, r + pad
    aligned16 = (ldu * size) % 16 == 0 and (off * size) % 16 == 0
    if r > MAX_R:
        ng = 16 if init or r <= 256 else 32 if r <= 512 else 64
        return f'wide-NG{ng}-{"vec" if r % GROUP == 0 and aligned16 else "scalar"}'
    if (init or dt is np.float32) and r % GROUP == 0 and aligned16:
        return f'direct-NG{r // GROUP}'
    pair = r % 2 == 0 and ldu % 2 == 0 and (off * size) % (2 * size) == 0
    mtr = round_mt(r)
    return f'mfma-MTR{mtr}-LM{(2 if r == GROUP * mtr else 1) if pair else 0}'


def step_family(r):
    if r > MAX_R:
        return 'three-launch'
    lpr = 1
    while lpr < (r + 1) // 2:
        lpr *= 2
    return f'fused-LPR{lpr}-orth-NJ{1 if r <= 16 else 2 if r <= 32 else 4 if r <= 64 else 8}'


def sweep_cases():
    """(n, r, layout): every r meets every layout at N_TABLE rows, every row count meets ROWS_R (f64 and f32), and the
    grid-stride size"""
    cases = [(N_TABLE, r, lay) for r in ALL_R for lay in LAYOUTS]
    cases += [(n, r, lay) for n in ROWS if n != N_TABLE for r in ROWS_R for lay in ('contig', 'f32')]
    cases += [(N_STRIDE, r, lay) for r, lay in STRIDE_CASES]
    return cases


def sweep_id(case, init):
    n, r, lay = case
    return f'n{n}-r{r}-{lay}-{sweep_family(r, lay, init)}'


# ---- bases ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def basis(n, r, f32=False, seed=0):
    """Random rows of varied length (0.5 .. 1.5), read-only; f32: rounded to float32 storage"""
    rng = np.random.default_rng(100003 * seed + 1009 * r + n)
    U = rng.standard_normal((n, r)) * (0.5 + rng.random((n, 1))) / math.sqrt(r)
    if f32:
        U = U.astype(np.float32)
    U.setflags(write=False)
    return U


def widen(U):
    return np.asarray(U, dtype=np.float64)


def layout_buffer(U, layout):
    """-> (flat buffer of the storage type, offset, ldu): U at buffer[offset + i ldu + k], NaN everywhere else"""
    dt, pad, off = LAYOUTS[layout]
    assert U.dtype == dt
    n, r = U.shape
    ldu = r + pad
    buf = np.full(off + n * ldu + SLACK, np.nan, dtype=dt)
    np.lib.stride_tricks.as_strided(buf[off:], (n, r), (ldu * buf.itemsize, buf.itemsize))[:] = U
    return buf, off, ldu


def refresh_picks(n, row0, nq, rng):
    """nq global rows: inside the shard, in another shard (below row0, at and beyond row0 + n) and -1, in turn"""
    kinds = [lambda: row0 + int(rng.integers(0, n)), lambda: -1, lambda: row0 + n, lambda: row0 + n + 7 + int(rng.integers(0, 50)),
             lambda: row0 + int(rng.integers(0, n))]
    if row0 > 0:
        kinds += [lambda: row0 - 1, lambda: int(rng.integers(0, row0))]
    return np.array([kinds[t % len(kinds)]() for t in range(nq)], dtype=np.int64)


def planted_norms(nrm, rng):
    """a tenth of the rows already at -1, a tenth at 0.0"""
    out = np.array(nrm, dtype=np.float64, copy=True)
    out[rng.random(len(out)) < 0.1] = -1.0
    out[rng.random(len(out)) < 0.1] = 0.0
    return out


def orthonormal_rows(k, r, seed):
    """k <= r orthonormal rows of length r"""
    Q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((r, k)))
    return np.ascontiguousarray(Q.T)


# ---- references -----------------------------------------------------------------------------------------------------------
def ref_init(Uw):
    """squared row norms of the stored values, long double"""
    return (np.asarray(widen(Uw), dtype=LD) ** 2).sum(axis=1)


def ref_apply(nrm_in, Uw, Qrows, picks, row0):
    """The refresh, literally: max(nrm_in - sum_j (u . q_j)^2, 0); rows below 0 stay -1; the rows picks - row0 inside
    [0, n) become -1 (other picks, and -1, are ignored).  Long double."""
    nrm_in = np.asarray(nrm_in, dtype=LD)
    d = np.asarray(widen(Uw), dtype=LD) @ np.asarray(Qrows, dtype=LD).T
    out = np.maximum(nrm_in - (d * d).sum(axis=1), LD(0))
    out[nrm_in < 0] = -1
    for g in np.asarray(picks, dtype=np.int64):
        if g >= 0 and 0 <= g - row0 < len(out):
            out[g - row0] = -1
    return out


def gs_ld(v, Qprev):
    """two Gram-Schmidt passes against the rows of Qprev, normalised, long double"""
    v = np.array(v, dtype=LD)
    Qp = np.asarray(Qprev, dtype=LD).reshape(-1, v.shape[0])
    for _ in range(2):
        v = v - Qp.T @ (Qp @ v)
    nn = np.sqrt(v @ v)
    return v / nn if nn > 0 else np.zeros_like(v)


def ref_step(recs, taus, first, Qprev):
    """One step on the stacked records (ranks, r + 3) and bounds -> dict(w, piv, gap, ok, q): the winner has the largest
    value, then the lowest global row; gap = (best - max(its runner-up, the other records' bests)) / best, 0 when
    best <= 0; ok = first or best > max(taus)"""
    c = np.asarray(recs, dtype=LD).reshape(-1, np.asarray(recs).shape[-1])
    w = int(np.lexsort((c[:, 1], -c[:, 0]))[0])
    best = c[w, 0]
    second = max([c[w, 2]] + [c[i, 0] for i in range(c.shape[0]) if i != w])
    gap = (best - second) / best if best > 0 else LD(0)
    ok = bool(first) or bool(best > np.max(np.asarray(taus, dtype=LD)))
    return dict(w=w, piv=int(c[w, 1]), gap=gap, ok=ok, q=gs_ld(c[w, 3:], Qprev))


def sweep_grid(n, cap=MAX_BLOCKS):
    """workgroups of a sweep (sweep_grid of qr_pivot.hip); cap = device_cap(CUs)"""
    return min(-(-n // PANEL), cap)


def device_cap(cus):
    return min(4 * cus, MAX_BLOCKS)


def candidate_model(nrm, row0, grid):
    """The documented candidate rule (include/spr_hip.h, K6; header of qr_pivot.hip): workgroup b sweeps the panels
    b, b + grid, ... and keeps its TOPT best rows -- value descending, then lowest row; tau = the largest TOPT-th best value
    over the workgroups, -2.0 when no workgroup has TOPT rows.  -> (local rows of the candidate slots in workgroup order, tau);
    rows at -1 take slots like any other (the record leaves them out)."""
    nrm = np.asarray(nrm)
    n = len(nrm)
    npan = -(-n // PANEL)
    cand, tau = [], -2.0
    for b in range(grid):
        rows = np.concatenate([np.arange(c * PANEL, min((c + 1) * PANEL, n)) for c in range(b, npan, grid)])
        keep = rows[np.lexsort((rows, -nrm[rows]))][:TOPT]
        cand.append(keep)
        if len(keep) == TOPT:
            tau = max(tau, float(nrm[keep[-1]]))
    return np.concatenate(cand), tau


def model_record(nrm, cand, row0, Uw):
    """best live candidate -> (value, global row, runner-up among the live candidates, its stored row widened)"""
    nrm = np.asarray(nrm)
    live = cand[nrm[cand] >= 0]
    if live.size == 0:
        return np.concatenate([[-2.0, 2.0 ** 63, -2.0], np.zeros(Uw.shape[1])])
    order = live[np.lexsort((live, -nrm[live]))]
    second = nrm[order[1]] if order.size > 1 else -2.0
    return np.concatenate([[nrm[order[0]], row0 + order[0], second], widen(Uw)[order[0]]]).astype(np.float64)


def tau_bounds(nrm, grid):
    """what any sound tau satisfies, whatever the panel deal: at most the TOPT-th largest norm, at least the
    (TOPT grid + 1)-th (some row of the TOPT grid + 1 largest is no candidate); (-2, -2) below TOPT rows"""
    s = np.sort(np.asarray(nrm))[::-1]
    if len(s) < TOPT:
        return -2.0, -2.0
    return (float(s[TOPT * grid]) if len(s) > TOPT * grid else -2.0), float(s[TOPT - 1])


def greedy_trace_ld(U, s):
    """Greedy max-residual pivoting in long double, lowest index among equals -> dict(piv, gap (relative lead of every
    pick), frac (the winner's residual norm^2 over its row's norm^2), Q)"""
    Uw = np.asarray(widen(U), dtype=LD)
    nrm0 = (Uw ** 2).sum(axis=1)
    nrm = nrm0.copy()
    Q = np.zeros((s, Uw.shape[1]), dtype=LD)
    piv, gap, frac = [], [], []
    for j in range(s):
        p = int(np.argmax(nrm))
        best = nrm[p]
        second = np.max(np.delete(nrm, p)) if len(nrm) > 1 else LD(-2)
        piv.append(p)
        gap.append(float((best - second) / best) if best > 0 else 0.0)
        frac.append(float(best / nrm0[p]) if nrm0[p] > 0 else 0.0)
        Q[j] = gs_ld(Uw[p], Q[:j])
        d = Uw @ Q[j]
        new = np.maximum(nrm - d * d, LD(0))
        new[nrm < 0] = -1
        new[p] = -1
        nrm = new
    return dict(piv=np.asarray(piv, dtype=np.int64), gap=np.asarray(gap), frac=np.asarray(frac), Q=Q)


def greedy_pivots_ld(U, s):
    t = greedy_trace_ld(U, s)
    return t['piv'], t['gap']


def model_batch(nrm, Uw, row0, grid, Qprev, nb, first):
    """nb steps on the candidate set of `nrm` (float64, as a sweep left it), long double: what qr_steps computes between
    two sweeps.  -> dict(tau, piv (global), gap, ok, lead (|best - tau| / best), frac, Q (nb directions), rec_row /
    rec_val / rec_second / rec_gap / rec_frac: the best remaining candidate afterwards)"""
    Uw = widen(Uw)
    cand, tau = candidate_model(nrm, row0, grid)
    cand = cand[np.asarray(nrm)[cand] >= 0]
    res = np.asarray(nrm, dtype=LD)[cand]
    Uc = np.asarray(Uw[cand], dtype=LD)
    nrm0 = (Uc ** 2).sum(axis=1)
    Qs = [np.asarray(q, dtype=LD) for q in np.asarray(Qprev).reshape(-1, Uw.shape[1])]
    out = dict(tau=tau, piv=[], gap=[], ok=[], lead=[], frac=[], Q=[])

    def best_two():
        live = np.flatnonzero(res >= 0)
        order = live[np.lexsort((cand[live], -res[live]))]
        return (int(order[0]) if order.size else -1), (res[order[1]] if order.size > 1 else LD(-2))

    w, second = best_two()
    for t in range(nb):
        best = res[w]
        out['piv'].append(int(row0 + cand[w]))
        out['gap'].append(float((best - second) / best) if best > 0 else 0.0)
        out['ok'].append(bool(t == 0 and first) or bool(best > tau))
        out['lead'].append(abs(float((best - LD(tau)) / best)) if best > 0 else 0.0)
        out['frac'].append(float(best / nrm0[w]) if nrm0[w] > 0 else 0.0)
        q = gs_ld(Uc[w], np.array(Qs, dtype=LD) if Qs else np.zeros((0, Uw.shape[1]), dtype=LD))
        Qs.append(q)
        out['Q'].append(q)
        d = Uc @ q
        new = np.maximum(res - d * d, LD(0))
        new[res < 0] = res[res < 0]
        new[w] = -1
        res = new
        w, second = best_two()
    out.update(rec_row=int(row0 + cand[w]) if w >= 0 else None, rec_val=res[w] if w >= 0 else LD(-2), rec_second=second,
               rec_gap=float((res[w] - second) / res[w]) if w >= 0 and res[w] > 0 else 0.0,
               rec_frac=float(res[w] / nrm0[w]) if w >= 0 and nrm0[w] > 0 else 0.0)
    return out


def record_is_decided(b):
    """the best remaining candidate after a batch can be told from the references: one is left, and its residual is still a
    tenth of its row (what is left of a basis whose span is exhausted is rounding noise)"""
    return b['rec_row'] is not None and math.sqrt(b['rec_frac']) >= 0.1


# ---- bars -----------------------------------------------------------------------------------------------------------------
def init_bar(Uw):
    return (Uw.shape[1] + 2) * U_RND * ref_init(Uw)


def apply_bar(Uw, nq):
    r = Uw.shape[1]
    return 2 * ((2 * r + 1) * math.sqrt(nq) + nq + 2) * U_RND * ref_init(Uw)


GAP_BAR = 4 * U_RND                               # relative


# ---- group 4: the step cases ------------------------------------------------------------------------------------------------
STEP_ROW0 = 1000
STEP_CALLS = (1, 2, QR_BATCH)                     # steps per call, then QR_BATCH again and again up to step_count(r)


def step_count(r):
    """steps taken on the basis of width r: three calls (19 steps), every step at r = 16 (steps 0 .. 15) and r = 64 (steps
    60 .. 63 reach the last rows of the direction tile)"""
    return r if r in (16, 64) else min(r, sum(STEP_CALLS))


@functools.lru_cache(maxsize=None)
def step_basis(r):
    """basis(N_TABLE, r); above 64 columns these fall off by 0.93 each, so that the winners come down to tau within the
    steps taken (a certified prefix k < nb on the widest fused step and on the three-launch path as well) while a residual
    keeps 0.93^(2 x 19) = 0.06 of its row"""
    U = np.array(basis(N_TABLE, r, seed=4))
    if r > 64:
        U *= 0.93 ** np.arange(r)
    U.setflags(write=False)
    return U


@functools.lru_cache(maxsize=None)
def step_protocol(r):
    """The driver's protocol on step_basis(r) in long double with the candidate model: calls of STEP_CALLS steps, the
    certified prefix k of each accepted, a refresh with those k directions.  -> list of dict(j, nb, k, batch)"""
    U = step_basis(r)
    grid = sweep_grid(N_TABLE)
    nrm = ref_init(U).astype(np.float64)
    Q = np.zeros((0, r), dtype=LD)
    calls, j, sizes = [], 0, list(STEP_CALLS)
    while j < step_count(r):
        nb = min(sizes.pop(0) if sizes else QR_BATCH, step_count(r) - j)
        b = model_batch(nrm, U, STEP_ROW0, grid, Q, nb, True)
        k = nb if all(b['ok']) else b['ok'].index(False)
        calls.append(dict(j=j, nb=nb, k=k, batch=b))
        Qk = np.array(b['Q'][:k], dtype=LD)
        nrm = ref_apply(nrm, U, Qk, b['piv'][:k], STEP_ROW0).astype(np.float64)
        Q = np.concatenate([Q, Qk])
        j += k
    return calls


@functools.lru_cache(maxsize=None)
def twin_direction_errors(r):
    """NumpyEngine.qr_step (float64, the device's algorithm) on step_basis(r), every direction against the long-double
    Gram-Schmidt of the same row against the double's own earlier directions -> worst (|q - ref|_inf, | |q| - 1 |,
    |Q[:step] q|_inf) over the steps"""
    U = np.array(step_basis(r))
    eng = NumpyEngine()
    s = step_count(r)
    st = eng.qr_begin(torch.from_numpy(U), STEP_ROW0, s)
    worst = np.zeros(3)
    for step in range(s):
        row = st['rec'].numpy()[3:].copy()
        eng.qr_step(st, step, st['rec'][None], st['tau'][None], True)
        worst = np.maximum(worst, direction_errors(st['Q'].numpy(), step, row))
    return tuple(float(x) for x in worst)


def direction_errors(Q, step, row):
    """(|q - ref|_inf, | |q| - 1 |, |Q[:step] q|_inf) of Q[step], ref = gs_ld(row, Q[:step]), measured in long double"""
    q = np.asarray(Q[step], dtype=LD)
    ref = gs_ld(row, Q[:step])
    Qp = np.asarray(Q[:step], dtype=LD)
    return np.array([float(np.max(np.abs(q - ref))), float(abs(np.sqrt(q @ q) - 1)),
                     float(np.max(np.abs(Qp @ q))) if step else 0.0])


def twin_worst():
    """the double's worst values over the whole case list"""
    return tuple(np.max([twin_direction_errors(r) for r in ALL_R], axis=0))


# ---- group 3: exact bases ---------------------------------------------------------------------------------------------------
EXACT_R = (4, 16, 64)
EXACT_N = (65, 323, 1000)
EXACT_SPOTS = ('middle', 'panel-start', 'last-panel-start', 'last-row')


def exact_basis(n, r, spot, f32=False):
    """Entries +-1.  Every row has norm^2 r; after the first pick (row 0) the residual of row i is r - (u_i . u_0)^2 / r, exact in
    float64 in any summation order.  Rows orthogonal to u_0 keep the maximum r: they are planted at `spot` (the lowest of them)
    and, where a later row exists, a few rows behind it; every other row has u_i . u_0 != 0.  -> (U, lowest planted row, number of
    planted rows)"""
    rng = np.random.default_rng(17 * n + r)
    U = np.where(rng.random((n, r)) < 0.5, -1.0, 1.0)
    dot = U[1:] @ U[0]
    U[1:, 0] = np.where(dot == 0, -U[1:, 0], U[1:, 0])       # no accidental orthogonal row
    last = PANEL * ((n - 1) // PANEL)
    p = {'middle': n // 2 + 1, 'panel-start': PANEL * max(1, (n // PANEL) // 2), 'last-panel-start': last, 'last-row': n - 1}[spot]
    planted = sorted({p, min(p + 3, n - 1), min(p + PANEL + 5, n - 1)})
    for i in planted:
        U[i] = U[0]
        U[i, :r // 2] *= -1.0
    U = U.astype(np.float32) if f32 else U
    U.setflags(write=False)
    return U, p, len(planted)


def exact_residuals(U):
    """norms after the first step and its refresh, exactly: r - (u_i . u_0)^2 / r (integers over a power of two), row 0 at -1"""
    Uw = widen(U)
    r = Uw.shape[1]
    d = Uw @ Uw[0]
    out = r - d * d / r
    out[0] = -1.0
    return out


# ---- group 5: a planted basis whose second pivot is no candidate ------------------------------------------------------------
PLANT_N, PLANT_DECOYS, PLANT_EVERY = 640, 600, 16
PLANT_R = (8, 50)
PLANT_R_POOLS = 32                                # a width the epoch sweeps take: the pooled driver on the same plant


@functools.lru_cache(maxsize=None)
def planted_basis(r):
    """PLANT_DECOYS decoy rows c_i e_1 + 1e-3 noise elsewhere, c_i in [9, 11] all distinct, and 40 true rows of norm about 1
    inside e_2 .. e_r, one every PLANT_EVERY rows: every panel holds 60 decoys, so every candidate of the initial sweep is a
    decoy; after the first step the decoys collapse to about 1e-6 and the second pivot, a true row, is no candidate."""
    rng = np.random.default_rng(5000 + r)
    n = PLANT_N
    true = np.arange(PLANT_EVERY // 2 - 1, n, PLANT_EVERY)
    decoy = np.setdiff1d(np.arange(n), true)
    assert len(decoy) == PLANT_DECOYS
    U = np.zeros((n, r))
    U[decoy, 0] = 9.0 + 2.0 * rng.permutation(PLANT_DECOYS) / (PLANT_DECOYS - 1)
    U[decoy, 1:] = 1e-3 * rng.standard_normal((PLANT_DECOYS, r - 1))
    T = rng.standard_normal((len(true), r - 1))
    U[true, 1:] = T / np.linalg.norm(T, axis=1, keepdims=True) * (0.8 + 0.4 * rng.random((len(true), 1)))
    U.setflags(write=False)
    return dict(U=U, true=true, decoy=decoy, s=min(r, 30))


def check_planted(case):
    """the conditions the planted basis was built for, from the references alone -> the long-double pivots"""
    U, true, decoy = case['U'], case['true'], case['decoy']
    n = len(U)
    is_decoy = np.isin(np.arange(n), decoy)
    for c in range(-(-n // PANEL)):
        assert is_decoy[c * PANEL:(c + 1) * PANEL].sum() >= TOPT
    grid = sweep_grid(n)
    nrm = ref_init(U).astype(np.float64)
    cand, tau = candidate_model(nrm, 0, grid)
    assert is_decoy[cand].all() and 81.0 <= tau <= 121.0
    t = greedy_trace_ld(U, case['s'])
    assert t['gap'].min() >= DECISIVE
    assert is_decoy[t['piv'][0]] and not is_decoy[t['piv'][1:]].any()
    after = ref_apply(nrm, U, t['Q'][:1], t['piv'][:1], 0)
    assert float(after[decoy].max()) < 1e-3 and float(after[true].max()) > 0.5
    b = model_batch(nrm, U, 0, grid, np.zeros((0, U.shape[1])), 2, True)
    assert b['ok'] == [True, False] and b['piv'][0] == t['piv'][0] and b['piv'][1] != t['piv'][1]
    return t['piv']


# ---- group 6: two shards ----------------------------------------------------------------------------------------------------
SHARD_SPLITS = (64, 100, 322)
SHARD_R = ROWS_R


@functools.lru_cache(maxsize=None)
def shard_basis(r, tie=False):
    """step_basis(r); tie: the row of largest norm duplicated across every split (rows 40 and 322)"""
    U = np.array(step_basis(r))
    if tie:
        U[40] = 2.0 * U[np.argmax((U ** 2).sum(axis=1))]
        U[N_TABLE - 1] = U[40]
    U.setflags(write=False)
    return U


def shard_steps(r):
    return min(r, 8)


# ---- CPU checks -------------------------------------------------------------------------------------------------------------
def test_long_double_is_wider_than_double():
    assert np.finfo(LD).eps <= 2.0 ** -63


def test_every_kernel_family_is_reached():
    """the tables reach every instantiation launch_refresh and the steps select"""
    init = {sweep_family(r, lay, True) for _, r, lay in sweep_cases()}
    refresh = {sweep_family(r, lay, False) for _, r, lay in sweep_cases()}
    for ng in range(1, 9):
        assert f'direct-NG{ng}' in init and f'direct-NG{ng}' in refresh             # refresh: f32 storage
    for mtr in (1, 2, 3, 4, 6, 8):
        for lm in (0, 1, 2):
            assert f'mfma-MTR{mtr}-LM{lm}' in refresh, (mtr, lm)
        assert f'mfma-MTR{mtr}-LM0' in init                   # init takes the LDS form only where the direct form cannot run
    assert {'wide-NG16-vec', 'wide-NG16-scalar'} <= init
    assert {f'wide-NG{ng}-{v}' for ng in (16, 32, 64) for v in ('vec', 'scalar')} <= refresh
    steps = {step_family(r) for r in ALL_R}
    assert {f'fused-LPR{lpr}' for lpr in (1, 2, 4, 8, 16, 32, 64)} == {s.split('-orth')[0] for s in steps if s != 'three-launch'}
    assert {f'NJ{nj}' for nj in (1, 2, 4, 8)} == {s.split('orth-')[1] for s in steps if s != 'three-launch'}
    assert 'three-launch' in steps


def test_candidate_model_on_small_vectors():
    nrm = np.arange(200, dtype=np.float64)
    cand, tau = candidate_model(nrm, 0, sweep_grid(200))
    assert sorted(cand[:TOPT]) == list(range(PANEL - TOPT, PANEL)) and len(cand) == 3 * TOPT + 200 - 3 * PANEL
    assert tau == 3 * PANEL - TOPT                                      # the third panel's TOPT-th best; the last has 8 rows
    assert candidate_model(np.ones(TOPT - 1), 0, 1)[1] == -2.0
    cand, tau = candidate_model(np.ones(N_STRIDE), 0, MAX_BLOCKS)      # ties: the lowest rows, second panel never needed
    assert tau == 1.0 and (cand[:TOPT] == np.arange(TOPT)).all()
    lo, hi = tau_bounds(nrm, 4)
    assert lo <= candidate_model(nrm, 0, 4)[1] <= hi
    rec = model_record(np.array([3.0, -1.0, 3.0, 2.0]), np.array([0, 1, 2, 3]), 10, np.eye(4))
    assert rec[:3].tolist() == [3.0, 10.0, 3.0] and rec[3:].tolist() == [1.0, 0.0, 0.0, 0.0]


@pytest.mark.parametrize('r', ALL_R)
def test_step_cases_are_decisive(r):
    """group 4's basis: decisive leads among the candidates and against tau, winners' residuals at least 0.1 of their rows,
    the accepted picks are the long-double greedy order -- and LAPACK's"""
    calls = step_protocol(r)
    piv = []
    for c in calls:
        b = c['batch']
        upto = min(c['k'] + 1, c['nb'])                       # the accepted steps and the one that was refused
        assert min(b['gap'][:upto]) >= DECISIVE and min(b['lead'][:upto]) >= DECISIVE, (r, c['j'])
        assert min(np.sqrt(b['frac'][:upto])) >= 0.1, (r, c['j'], b['frac'])
        assert c['k'] >= 1
        if c['k'] == c['nb'] and record_is_decided(b):     # the record a fully certified call leaves behind
            assert b['rec_gap'] >= DECISIVE, (r, c['j'])
        piv += b['piv'][:c['k']]
    s = step_count(r)
    assert len(piv) == s
    want, gaps = greedy_pivots_ld(step_basis(r), s)
    assert gaps.min() >= DECISIVE
    np.testing.assert_array_equal(np.asarray(piv) - STEP_ROW0, want)
    np.testing.assert_array_equal(want, orc.qr_pivots(np.array(step_basis(r)))[0][:s])
    print(f'r = {r}: {step_family(r)}, calls (j, nb, k) = {[(c["j"], c["nb"], c["k"]) for c in calls]}')


def test_some_step_case_has_an_uncertified_tail():
    for r in ALL_R:
        if r >= 16:
            assert any(c['k'] < c['nb'] for c in step_protocol(r)), r


@pytest.mark.parametrize('n,r,f32', [(n, r, f32) for n in (17, 200, N_TABLE) for r in ROWS_R for f32 in (False, True)])
def test_greedy_ld_equals_lapack(n, r, f32):
    U = basis(n, r, f32)
    s = min(n, r)
    piv, gap = greedy_pivots_ld(U, s)
    k = int(np.argmax(gap < DECISIVE)) if (gap < DECISIVE).any() else s
    assert k >= min(s, 3)
    np.testing.assert_array_equal(piv[:k], orc.qr_pivots(widen(U))[0][:k])


@pytest.mark.parametrize('r', ALL_R)
def test_numpy_engine_step_vs_ref_step(r):
    """the float64 double against ref_step on its own records: same winner and flag, gap to 4 u, and the direction errors
    that set the device's bar"""
    U = np.array(step_basis(r))
    eng = NumpyEngine()
    s = step_count(r)
    st = eng.qr_begin(torch.from_numpy(U), STEP_ROW0, s)
    for step in range(s):
        recs, taus = st['rec'][None].numpy().copy(), st['tau'][None].numpy().copy()
        eng.qr_step(st, step, st['rec'][None], st['tau'][None], step == 0)
        want = ref_step(recs, taus, step == 0, st['Q'].numpy()[:step])
        assert int(st['piv'][step]) == want['piv'] and bool(st['ok'][step]) == want['ok']
        assert abs(LD(float(st['gap'][step])) - want['gap']) <= GAP_BAR * abs(want['gap'])
    e = twin_direction_errors(r)
    print(f'r = {r}: double |q - ref| {e[0]:.2e}  ||q| - 1| {e[1]:.2e}  |Q q| {e[2]:.2e}')
    assert max(e) < 1e-12


def test_twin_worst_values():
    w = twin_worst()
    print(f'double, worst over the case list: |q - ref| {w[0]:.3e}  ||q| - 1| {w[1]:.3e}  |Q q| {w[2]:.3e}')
    assert 0 < max(w) < 1e-12


@pytest.mark.parametrize('r,f32', [(r, f32) for r in ROWS_R + (128,) for f32 in (False, True)])
def test_numpy_engine_apply_vs_ref_apply(r, f32):
    rng = np.random.default_rng(r)
    U = basis(200, r, f32)
    nq = min(r, 7)
    Q = orthonormal_rows(nq, r, r)
    picks = refresh_picks(200, 1000, nq, rng)
    nrm = planted_norms(ref_init(U).astype(np.float64), rng)
    st = dict(nrm=torch.from_numpy(nrm.copy()), Ur=torch.from_numpy(np.array(U)), row0=1000, n=200, r=r)
    NumpyEngine().qr_apply(st, torch.from_numpy(Q), torch.from_numpy(picks))
    got, want = st['nrm'].numpy(), ref_apply(nrm, U, Q, picks, 1000)
    assert (np.abs(got - want) <= apply_bar(U, nq)).all()
    assert ((got == -1.0) == (want == -1)).all() and (got[(nrm == 0.0) & (want != -1)] == 0.0).all()
    cand, _ = candidate_model(got, 1000, sweep_grid(200))
    np.testing.assert_array_equal(st['rec'].numpy(), model_record(got, cand, 1000, U))


@pytest.mark.parametrize('r', PLANT_R + (PLANT_R_POOLS,))
def test_planted_basis_has_a_non_candidate_second_pivot(r):
    case = planted_basis(r)
    piv = check_planted(case)
    np.testing.assert_array_equal(piv, orc.qr_pivots(np.array(case['U']))[0][:case['s']])


@pytest.mark.parametrize('n', EXACT_N)
@pytest.mark.parametrize('r', EXACT_R)
@pytest.mark.parametrize('spot', EXACT_SPOTS)
def test_exact_bases(n, r, spot):
    U, p, count = exact_basis(n, r, spot)
    assert (ref_init(U) == r).all()
    res = exact_residuals(U)
    assert res.max() == r and int(np.argmax(res)) == p and int((res == r).sum()) == count
    assert (res[1:] * r == np.round(res[1:] * r)).all()
    want = ref_apply(np.full(n, float(r)), U, widen(U)[:1] / math.sqrt(r), [0], 0)
    assert (want == res).all()
    if spot == 'panel-start':
        assert p % PANEL == 0 and p > 0
    if spot == 'last-panel-start':
        assert p == PANEL * ((n - 1) // PANEL)
    if spot == 'last-row':
        assert p == n - 1 and count == 1


@pytest.mark.parametrize('r', SHARD_R)
def test_shard_cases_are_decisive(r):
    s = shard_steps(r)
    assert greedy_pivots_ld(shard_basis(r), s)[1].min() >= DECISIVE
    piv, gap = greedy_pivots_ld(shard_basis(r, tie=True), s)
    assert piv[0] == 40 and gap[0] == 0.0 and gap[1:].min() >= DECISIVE
