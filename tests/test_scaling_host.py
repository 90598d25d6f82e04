"""Every scaling and centring of ROM.scale_data / fit against a plain np.longdouble restatement of the reference's lines
106-169, on the NumPy engine double.  This file holds what tests/test_scaling_gpu.py shares with it: the data maker, the
longdouble reference, the bars and the check functions, which take the engine as an argument.  Run here, they test the
reference and the host half (ROM._merge_stats, _feature_scale, _feature_median); run there, the device code.

DATA.  F = 4 features, means (0.3, 7, 120, 2500) and spreads (2, 0.05, 11, 40) ('positive'); 'signed' makes the first and
the last mean negative: feature 0 then has a negative mean and values of both signs, feature 3 only negative values.  Every
feature is spread x [r - 1 modes L_f R with weights 0.95^j + a rank-one component g_i h_j whose g runs through the quantiles of
an exponential law (skewed: the median is not the mean) + 1 % noise], normalised to zero mean and unit variance; R and h are
shared by the features, so under every scaling X0 has r directions above the noise.  test_the_eleven_scalings_are_told_apart asserts that any two of the eleven
scale factors of a feature differ by 1e-3 relative: a swapped label cannot hide inside a bar.

THE BARS (u = 2^-53; stated before the first GPU run; n_p = n_points, N = n_p m values per feature, A_i = mean_j |x_ij|,
A_f = mean |x| of the block, amax_f = max |x|, sd_f its standard deviation).
* X_cnt, axis_cnt = 1 / -1: a row mean is a sum of m terms in any order and one division: m u A_i.
* Block mean mu_f (X_cnt with axis_cnt = None, and the input of 'vast', 'level', 'poisson', 'l2-norm'): the mean of n_p row
  means (m u A_i each), merged pairwise or one by one with four roundings per item (d = b - mu, d * nb, / tot, mu +):
  (m + 4 (n_p + ranks)) u A_f.
* Block variance var_f = (trace G_f + m M2_f) / (n_p m), G_f the Gram block of the row-centred values, M2_f the sum of squares
  of the row means about mu_f.  The identity is exact for ANY row centres a_i only with the cross term 2 m sum_i (a_i - mu)
  (mean_i - a_i); with a_i = mean_i + delta_i, |delta_i| <= m u A_i, dropping it costs 2 m sum_i |d_i| m u A_i (d_i = mean_i -
  mu_f), relative to N var_f: 2 m u cross_f, cross_f = sum_i |d_i| A_i / (n_p var_f) (<= amax_f / sd_f).  The sums themselves: a
  diagonal Gram entry is a sum of n_p squares (n_p u), the trace of m of them (m u), three roundings per term; M2 is merged with
  at most six roundings per item: together <= (4 n_p + m + 8 + 6 ranks) u.  rel_var = (4 n_p + m + 8 + 6 ranks) u + 2 m u cross_f.
* Scales, relative: std rel_var / 2 + u; pareto rel_var / 4 + 2 u; variance rel_var; vast rel_var + rel_mu + u; level
  rel_mu; poisson rel_mu / 2 + u; l2-norm = sqrt(N (var + mu^2)): (var rel_var + 2 mu^2 rel_mu) / (2 (var + mu^2)) + 4 u;
  none: exactly 1; max: exact (a maximum does not round); range and median: one rounding on either side, 2 u.
* X0 = (x - X_cnt) inv, inv = 1 / X_scl: bar_cnt / |scl| + |X0| (rel_scl + 3 u) entrywise (subtraction, reciprocal, product).
* unscale_data(X0[:, j]) returns (x - c)(1 + 4 roundings) + c, c the COMPUTED centre, whose own error cancels:
  4 u (|x - cnt| + bar_cnt) + 2 u |x|.  With a sampling matrix S: sum_k |S_ik| bar_cnt_k + |x0_i| sum_k |S_ik scl_k| rel_scl_k
  + (nnz_i + 2) u (|x0_i| sum_k |S_ik scl_k| + sum_k |S_ik cnt_k|).
* Sigma_r and the fields (Gram route).  The computed Gram matrix is that of a perturbed X0 plus dG.  The perturbations of X0:
  (a) the scale, rows of feature f times (1 + rho_f), |rho_f| <= rel_scl_f: multiplicative, sigma_i moves by <= max rho sigma_i
  (Ostrowski); (b) the centre, c 1^T with |c_i| <= bar_cnt_i / |scl|: 2-norm <= |c|_2 sqrt(m); (c) the three roundings of an
  entry, 3 u |X0|_F.  dG: the rounding of n = F n_p products per entry, (n + 2) u |X0|^T |X0| with 2-norm <= (n + 2) u |X0|_F^2,
  and the backward error of a symmetric eigen-solver, c m u sigma_1^2 with c = 4 (Jacobi and LAPACK alike; the NumPy engine sits
  at 16 u sigma_1^2 / sigma_i).  With axis_cnt = None the row-centred blocks are corrected by v 1^T + 1 v^T + M2 1 1^T, v = w -
  mu z from the column sums z = sum_i c_i, w = sum_i mean_i c_i, which cancel: e_v = (n_p + 4) u sum_i (|mean_i| + |mu|) |c_ij| per
  entry of v (2 sqrt(m) |e_v|_2 in norm), e_M2 = (4 n_p + 8) u M2 times m for the last term, both over scl^2, added to dG.
  |d sigma_i| <= max rho sigma_i + |c|_2 sqrt(m) + 3 u |X0|_F + dG / (2 sigma_i) + m u sigma_1, the last for the LAPACK SVD of
  the reference X0 rounded to float64.  This is the issue's c m u sigma_1^2 / sigma_i with the constants spelt out.
* Fields.  reconstruct(Ar[j]) is column j of X0 V_r V_r^T, unscaled.  The data have exactly r directions above 1 % noise, shared
  by the features, so the gap behind sigma_r is wide under every scaling.  Davis-Kahan (sin Theta theorem): the leading right
  singular subspace turns by sin_t <= |V_perp^T dA V_r|_2 / (lambda_r - lambda_{r+1} - 2 |dA|_2), dA the whole perturbation of
  the Gram matrix -- only its block between the two subspaces counts.  That block, term by term (p1 = |V_r^T 1|, q1 = |V_perp^T
  1|): (a) 2 rho_f V_perp^T G_f V_r <= 2 rho_f |X0_f V_perp|_2 |X0_f V_r|_2, small because the features share their row space;
  (b) row centring: |c|_2 (sigma_{r+1} p1 + sigma_1 q1); scalar centring, where c is one number d_f per feature: d_f (|V_perp^T
  s_f| p1 + q1 |V_r^T s_f|), s_f the column sums of X0_f; (c) 2 sigma_1 3 u |X0|_F; dG's first two terms in full; e_v sqrt(m)
  (Cauchy-Schwarz over the two subspaces) and e_M2 p1 q1.  A projector moves by exactly sin_t in the 2-norm, so entry (i, j) of
  the scaled field moves by <= sin_t |X0_i|_2, the 2-norm of ROW i.  The projection U = X W - mean (1^T W) carries the raw values
  through its products: (m + r + 8) u sqrt(r) |x_i|_2 in the units of X.  Per row, in those units: sin_t |x_i - cnt_i|_2 + (m + r +
  8) u sqrt(r) |x_i|_2 + |scl_f| |E_i|_2 (the X0 bar of the row) + bar_cnt_i + max_j |scl_f field0_ij| (rel_scl + 3 u) + u max_j
  |field_ij|; checked entrywise and asserted below 1e-9 of the feature's LARGEST ENTRY (largest: 8.4e-10, (50, 600), 'variance',
  axis_cnt = None, feature 0, whose entries are the smallest against its row norms).
Every bar that is not exact is asserted to lie below 1e-9 of its quantity (assert_small)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sps
import torch

from oracle import spr_oracle as orc
from openmeasure_amd.sparse_sensing import SPR, DeviceMatrix
from tests.numpy_engine import NumpyEngine

LD = np.longdouble
U = 2.0 ** -53
F = 4
SCALINGS = ('std', 'none', 'pareto', 'vast', 'range', 'level', 'max', 'variance', 'median', 'poisson', 'l2-norm')
CODE_SCALINGS = ('std', 'none', 'pareto', 'vast', 'level', 'variance', 'poisson', 'l2-norm')
AXES = (1, -1, None)
MEANS = {'positive': (0.3, 7.0, 120.0, 2500.0), 'signed': (-0.3, 7.0, 120.0, -2500.0)}
SPREADS = (2.0, 0.05, 11.0, 40.0)
SHAPES = [(77, 7), (77, 24), (77, 25), (130, 65), (50, 300)]
WIDE = (50, 600)                                            # two 512-column launches of colsums: axis_cnt = None only
# (n_points, m, axis_cnt) of every case
CASES = [(n_p, m, ax) for (n_p, m) in SHAPES for ax in AXES] + [WIDE + (None,)]
IDS = [f'{n_p}x{m}-axis{ax}' for n_p, m, ax in CASES]


# ------------------------------------------------------------------------------------------------ data
@functools.lru_cache(maxsize=None)
def make_case(n_points, m, variant='positive', dtype='f64'):
    """(F n_points, m) snapshot matrix of the module docstring; the same fluctuations for both variants.  Shared: never
    written to."""
    rng = np.random.default_rng(1000 * n_points + m)
    k = (4 if m == 7 else 6) - 1                              # with h: as many directions as fit() is asked for
    R = (0.95 ** np.arange(k))[:, None] * rng.standard_normal((k, m))
    h = 1.0 + 0.6 * (rng.random(m) - 0.5)
    X = np.empty((F * n_points, m))
    for f in range(F):
        L = rng.standard_normal((n_points, k))
        g = rng.permutation(-np.log1p(-(np.arange(n_points) + 0.5) / n_points)) - 1.0   # the quantiles of an exponential law
        z = 0.3 * (L @ R) + np.outer(g, h) + 0.01 * rng.standard_normal((n_points, m))
        z = (z - z.mean()) / z.std()
        X[f * n_points:(f + 1) * n_points] = MEANS[variant][f] + SPREADS[f] * z
    return X.astype(np.float32) if dtype == 'f32' else X


def make_sampling(n):
    """CSR (9, n): seven rows with one entry (first and last row of the matrix among them), two with several entries that
    reach across features"""
    S = np.zeros((9, n))
    for i, row in enumerate([0, n - 1, n // 4, n // 4 - 1, n // 2 + 3, 17, n - n // 4]):
        S[i, row] = (1.0, 1.0, 0.5, 2.0, 1.0, -1.5, 1.0)[i]
    S[7, [1, n // 4 + 2, n // 2 + 1, n - 2]] = (0.25, 0.5, -0.125, 1.0)
    S[8, [n // 4 - 2, n // 4, n - 5]] = (1.0, -3.0, 0.75)
    return sps.csr_matrix(S)


# ------------------------------------------------------------------------------------------------ the longdouble reference
@functools.lru_cache(maxsize=None)
def block_stats(n_points, m, variant, dtype):
    """direct formulas on the stored values, widened to longdouble"""
    x = np.ascontiguousarray(make_case(n_points, m, variant, dtype)).astype(LD).reshape(F, n_points, m)
    N = LD(n_points * m)
    mean = x.sum(axis=(1, 2)) / N
    var = ((x - mean[:, None, None]) ** 2).sum(axis=(1, 2)) / N
    flat = x.reshape(F, -1)
    return dict(x=x, mean=mean, var=var, sd=np.sqrt(var), max=flat.max(axis=1), min=flat.min(axis=1),
                median=np.array([np.median(flat[f]) for f in range(F)], dtype=LD), l2=np.sqrt((flat * flat).sum(axis=1)),
                A=np.abs(flat).mean(axis=1), amax=np.abs(flat).max(axis=1), rowmean=x.sum(axis=2) / LD(m),
                rowabs=np.abs(x).sum(axis=2) / LD(m))


def ref_scale(st, scale_type):
    """reference :114-161, one factor per feature (NaN where the reference has it)"""
    with np.errstate(invalid='ignore'):
        return {'std': st['sd'], 'none': np.ones(F, dtype=LD), 'pareto': np.sqrt(st['sd']), 'vast': st['var'] / st['mean'],
                'range': st['max'] - st['min'], 'level': st['mean'], 'max': st['max'], 'variance': st['var'],
                'median': st['median'], 'poisson': np.sqrt(st['mean']), 'l2-norm': st['l2']}[scale_type]


def reference(n_points, m, variant, dtype, scale_type, axis_cnt, ranks=1):
    """X_cnt (n,), X_scl per feature (F,), X0 (n, m) in longdouble, and the bars of the module docstring"""
    st = block_stats(n_points, m, variant, dtype)
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    scl = ref_scale(st, scale_type)
    rows = np.repeat(np.arange(F), n_points)
    cnt = st['rowmean'].reshape(-1) if axis_cnt is not None else st['mean'][rows]
    with np.errstate(invalid='ignore'):
        X0 = (st['x'].reshape(F * n_points, m) - cnt[:, None]) / scl[rows][:, None]
    mu, var, sd, A = f64(st['mean']), f64(st['var']), f64(st['sd']), f64(st['A'])
    bar_mu = (m + 4 * (n_points + ranks)) * U * A
    rel_mu = bar_mu / np.abs(mu)
    cross = np.sum(np.abs(f64(st['rowmean'] - st['mean'][:, None])) * f64(st['rowabs']), axis=1) / (n_points * var)
    rel_var = (4 * n_points + m + 8 + 6 * ranks) * U + 2 * m * U * cross
    rel_scl = {'std': rel_var / 2 + U, 'none': 0 * mu, 'pareto': rel_var / 4 + 2 * U, 'vast': rel_var + rel_mu + U,
               'range': 0 * mu + 2 * U, 'level': rel_mu, 'max': 0 * mu, 'variance': rel_var, 'median': 0 * mu + 2 * U,
               'poisson': rel_mu / 2 + U,
               'l2-norm': (var * rel_var + 2 * mu * mu * rel_mu) / (2 * (var + mu * mu)) + 4 * U}[scale_type]
    bar_cnt = m * U * f64(st['rowabs']).reshape(-1) if axis_cnt is not None else bar_mu[rows]
    with np.errstate(invalid='ignore'):
        bar_X0 = bar_cnt[:, None] / np.abs(f64(scl))[rows][:, None] + np.abs(f64(X0)) * (rel_scl[rows][:, None] + 3 * U)
    return dict(st=st, rows=rows, cnt=cnt, scl=scl, X0=X0, bar_mu=bar_mu, rel_mu=rel_mu, rel_var=rel_var, rel_scl=rel_scl,
                bar_cnt=bar_cnt, bar_X0=bar_X0, finite=np.isfinite(f64(scl)))


def assert_small(name, rel):
    """every bar that is not exact lies below 1e-9 of its quantity"""
    rel = float(np.max(rel))
    assert rel < 1e-9, (name, rel)


def worst(err, bar):
    """largest error as a fraction of its bar; an exact bar (0) takes no error at all"""
    err, bar = np.asarray(err, dtype=np.float64), np.broadcast_to(np.asarray(bar, dtype=np.float64), np.shape(err))
    assert np.all(err <= bar), (float(np.max(err - bar)), float(np.max(err)), float(np.max(bar)))
    nz = bar > 0
    return float(np.max(err[nz] / bar[nz])) if nz.any() else 0.0


def wrap_host(X):
    return X


def wrap_column_slice(to_device):
    """X as a DeviceMatrix over columns [2, 2 + m) of a wider buffer: row stride m + 5"""
    def wrap(X):
        buf = np.full((X.shape[0], X.shape[1] + 5), 1e30, dtype=X.dtype)
        buf[:, 2:2 + X.shape[1]] = X
        t = to_device(buf)[:, 2:2 + X.shape[1]]
        assert t.stride(0) == X.shape[1] + 5
        return DeviceMatrix(t)
    return wrap


# ------------------------------------------------------------------------------------------------ 1. scale_data
def check_scale_data(eng, n_points, m, variant, dtype, scale_type, axis_cnt, wrap=wrap_host):
    """X_cnt, X_scl, X0, unscale_data with and without a sampling matrix against the longdouble reference"""
    X = make_case(n_points, m, variant, dtype)
    ref = reference(n_points, m, variant, dtype, scale_type, axis_cnt)
    rows, fin, st = ref['rows'], ref['finite'], ref['st']
    n = F * n_points
    spr = SPR(wrap(X), F, None, engine=eng)
    X0 = spr.scale_data(scale_type, axis_cnt)
    cnt, scl_rows = spr.X_cnt, spr.X_scl
    assert X0.shape == (n, m) and cnt.shape == scl_rows.shape == (n, 1) and X0.dtype == np.float64
    scl = scl_rows[::n_points, 0]
    assert np.array_equal(scl_rows[:, 0], scl[rows], equal_nan=True)                  # one factor per feature
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    assert np.array_equal(np.isnan(scl), np.isnan(f64(ref['scl']))), (scl, ref['scl'])  # NaN exactly where the reference has it
    assert np.array_equal(np.signbit(scl[fin]), np.signbit(f64(ref['scl'])[fin])), (scl, ref['scl'])
    if variant == 'positive' or scale_type != 'poisson':
        assert fin.all()
    else:
        assert not fin[0] and not fin[3] and fin[1] and fin[2]
    assert_small('cnt', ref['bar_cnt'] / f64(st['A'])[rows])
    assert_small('scl', ref['rel_scl'])
    out = {}
    out['cnt'] = worst(np.abs(cnt[:, 0] - ref['cnt']), ref['bar_cnt'])
    out['scl'] = worst(np.abs(scl[fin] - ref['scl'][fin]), ref['rel_scl'][fin] * np.abs(f64(ref['scl'])[fin]))
    rfin = fin[rows]
    assert np.isnan(X0[~rfin]).all() and np.isfinite(X0[rfin]).all()
    assert_small('X0', np.max(ref['bar_X0'][rfin]) / np.max(np.abs(f64(ref['X0'][rfin]))))
    out['X0'] = worst(np.abs(X0[rfin] - ref['X0'][rfin]), ref['bar_X0'][rfin])
    # unscale_data(X0[:, j]) gives column j of X back
    j = m // 2
    xw = st['x'].reshape(n, m)[:, j]
    x = spr.unscale_data(np.ascontiguousarray(X0[:, j]))
    assert x.shape == (n,) and np.isnan(x[~rfin]).all()
    bar_un = 4 * U * (f64(np.abs(xw - ref['cnt'])) + ref['bar_cnt']) + 2 * U * f64(np.abs(xw))
    assert_small('unscale', np.max(bar_un[rfin]) / np.max(np.abs(f64(xw[rfin]))))
    out['unscale'] = worst(np.abs(x[rfin] - xw[rfin]), bar_un[rfin])
    # unscale_data(x0_s, sampling=S) = (S X_scl) x0_s + S X_cnt
    S = make_sampling(n)
    x0_s = np.linspace(-1.5, 2.0, 9)
    xs = spr.unscale_data(x0_s, sampling=S)
    Sd = S.toarray().astype(LD)
    aS = np.abs(f64(Sd))
    with np.errstate(invalid='ignore'):
        dot = lambda v: np.array([np.sum(Sd[i, aS[i] > 0] * v[aS[i] > 0]) for i in range(9)])   # stored entries only, as CSR does
        want = dot(ref['scl'][rows]) * x0_s + dot(ref['cnt'])
        s_scl = aS @ np.nan_to_num(np.abs(f64(ref['scl'])))[rows]
        bar_s = (aS @ ref['bar_cnt'] + np.abs(x0_s) * (aS @ np.nan_to_num(np.abs(f64(ref['scl'])) * ref['rel_scl'])[rows])
                 + ((aS > 0).sum(axis=1) + 2) * U * (np.abs(x0_s) * s_scl + aS @ np.abs(f64(ref['cnt']))))
    sfin = np.isfinite(f64(want))
    assert xs.shape == (9,) and np.array_equal(np.isfinite(xs), sfin)
    assert_small('sampled', bar_s[sfin] / (np.abs(x0_s) * s_scl + aS @ np.abs(f64(ref['cnt'])))[sfin])   # of the sum of absolute terms
    out['sampled'] = worst(np.abs(xs[sfin] - want[sfin]), bar_s[sfin])
    print(f'scale_data {n_points}x{m} {variant} {dtype} {scale_type} axis_cnt={axis_cnt}: error / bar ' +
          ' '.join(f'{k} {v:.2f}' for k, v in out.items()))
    return spr, out


# ------------------------------------------------------------------------------------------------ 3. kernels on row windows
WINDOWS = [(77, 7, 30, 100), (77, 7, 100, 40), (130, 65, 5, 500), (50, 300, 60, 130), (50, 600, 20, 75), (50, 600, 110, 30)]


def check_kernels_on_window(eng, n_points, m, row0, n_loc, dtype):
    """scale_rows, unscale (both branches), fill_feature, feature_minmax and colsums on rows [row0, row0 + n_loc) of the
    signed matrix, against NumPy on the same rows"""
    X = make_case(n_points, m, 'signed', dtype)[row0:row0 + n_loc]
    xw = X.astype(np.float64)
    feat = (row0 + np.arange(n_loc)) // n_points
    assert row0 % n_points and (row0 + n_loc) % n_points                               # the window starts and ends inside features
    rng = np.random.default_rng(row0 + m)
    Xd = eng.to_device(X, dtype=torch.float32 if dtype == 'f32' else None)
    values = rng.standard_normal(F) * 10.0 ** np.arange(F)
    assert np.array_equal(eng.to_host(eng.fill_feature(n_loc, row0, n_points, eng.to_device(values))), values[feat])
    mm = eng.to_host(eng.feature_minmax(Xd, row0, n_points, F))
    want = np.array([(xw[feat == f].min(), xw[feat == f].max()) if np.any(feat == f) else (np.inf, -np.inf) for f in range(F)])
    assert np.array_equal(mm, want), (mm, want)
    mu = xw.mean(axis=1) + 0.01 * rng.standard_normal(n_loc)
    inv = 1.0 / (np.array([3.0, -0.07, 11.0, 1e3]) * (1.0 + rng.random(F)))
    mu_d = eng.to_device(mu)
    got = eng.to_host(eng.scale_rows(Xd, row0, n_points, F, mu_d, eng.to_device(inv)))
    assert np.array_equal(got, (xw - mu[:, None]) * inv[feat][:, None])
    x0, scale, rowscale = rng.standard_normal(n_loc), 1.0 / inv, rng.standard_normal(n_loc) * 5.0
    out = {}
    for name, rs in (('unscale', None), ('unscale rowscale', rowscale)):
        got = eng.to_host(eng.unscale(eng.to_device(x0), row0, n_points, F, mu_d, eng.to_device(scale),
                                      rowscale=None if rs is None else eng.to_device(rs)))
        s = scale[feat] if rs is None else rs
        bar_u = 2 * U * (np.abs(s * x0) + np.abs(mu))                                     # 1 ulp: fused or not
        assert_small(name, bar_u / (np.abs(s * x0) + np.abs(mu)))
        out[name] = worst(np.abs(got - (s.astype(LD) * x0 + mu)), bar_u)
    rowmean = xw.mean(axis=1)
    cs = eng.to_host(eng.colsums(Xd, row0, n_points, F, eng.to_device(rowmean)))
    assert cs.shape == (F, 2, m)
    d = xw.astype(LD) - rowmean.astype(LD)[:, None]
    for f in range(F):
        sel = feat == f
        nf = int(sel.sum())
        if not nf:
            assert np.all(cs[f] == 0.0)
            continue
        z, w = d[sel].sum(axis=0), (rowmean.astype(LD)[sel, None] * d[sel]).sum(axis=0)
        bz = (nf + 1) * U * np.abs(d[sel]).sum(axis=0).astype(np.float64)
        bw = (nf + 2) * U * np.abs(rowmean[sel, None] * d[sel]).sum(axis=0).astype(np.float64)
        assert_small('colsums', np.concatenate([bz / np.abs(d[sel]).sum(axis=0).astype(np.float64),
                                                bw / np.abs(rowmean[sel, None] * d[sel]).sum(axis=0).astype(np.float64)]))
        out['colsums z'] = max(out.get('colsums z', 0.0), worst(np.abs(cs[f, 0] - z), bz))
        out['colsums w'] = max(out.get('colsums w', 0.0), worst(np.abs(cs[f, 1] - w), bw))
    print(f'kernels {n_points}x{m} rows [{row0}, {row0 + n_loc}) {dtype}: error / bar ' + ' '.join(f'{k} {v:.2f}' for k, v in out.items()))
    return out


# ------------------------------------------------------------------------------------------------ 5. fit
@functools.lru_cache(maxsize=4)
def reference_svd(n_points, m, variant, dtype, scale_type, axis_cnt):
    ref = reference(n_points, m, variant, dtype, scale_type, axis_cnt)
    Uu, S, Vt = np.linalg.svd(np.asarray(ref['X0'], dtype=np.float64), full_matrices=False)
    return ref, Uu, S, Vt


def spectrum_bars(ref, S, Vt, n_points, m, axis_cnt, r):
    """The bar on Sigma_r and sin_t, the bound on the turn of the leading right singular subspace (module docstring)"""
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    st, rows = ref['st'], ref['rows']
    n = F * n_points
    X0, ascl, rho = f64(ref['X0']), np.abs(f64(ref['scl'])), ref['rel_scl']
    Vr, Vp = Vt[:r].T, Vt[r:].T
    s_next = S[r] if r < len(S) else 0.0
    p1 = np.linalg.norm(Vr.T @ np.ones(m))                                               # |V_r^T 1|, |V_perp^T 1|
    q1 = np.sqrt(max(m - p1 * p1, 0.0))
    fro = np.sqrt(float(np.sum(S * S)))
    cn = np.linalg.norm(ref['bar_cnt'] / ascl[rows])
    dG = (n + 2) * U * fro * fro + 4 * m * U * S[0] ** 2                                 # products and eigen-solver: full norm
    res = dG                                                                             # ... and as a bound on the residual block
    if axis_cnt is None:
        scl2 = ascl ** 2
        c = np.abs(f64(st['x'] - st['rowmean'][:, :, None]))                            # (F, n_p, m)
        rm = f64(st['rowmean'])
        e_v = (n_points + 4) * U * np.einsum('fi,fij->fj', np.abs(rm) + np.abs(f64(st['mean']))[:, None], c)
        e_v = float(np.sum(np.linalg.norm(e_v, axis=1) / scl2))
        e_m2 = float(np.sum((4 * n_points + 8) * U * np.sum((rm - f64(st['mean'])[:, None]) ** 2, axis=1) / scl2))
        dG += 2 * np.sqrt(m) * e_v + m * e_m2
        res += np.sqrt(m) * e_v + p1 * q1 * e_m2                                         # |V_perp^T e| p1 + q1 |V_r^T e| <= |e| sqrt(m)
    bar_S = np.max(rho) * S[:r] + cn * np.sqrt(m) + 3 * U * fro + dG / (2 * S[:r]) + m * U * S[0]
    for f in range(F):                                                                   # the scale: 2 rho_f V_perp^T G_f V_r
        Xf = X0[rows == f]
        res += 2 * rho[f] * (1 + rho[f]) * (np.linalg.norm(Xf @ Vp, 2) if Vp.shape[1] else 0.0) * np.linalg.norm(Xf @ Vr, 2)
    if axis_cnt is None:                                                                 # the centre: d_f e_f 1^T, e_f the feature's rows
        for f in range(F):
            col = X0[rows == f].sum(axis=0)                                              # X0^T e_f
            d = ref['bar_mu'][f] / ascl[f]
            res += d * (np.linalg.norm(Vp.T @ col) * p1 + q1 * np.linalg.norm(Vr.T @ col)) + d * d * n_points * p1 * q1
    else:                                                                                # c 1^T with any signs in c
        res += cn * (s_next * p1 + S[0] * q1) + cn * cn * p1 * q1
    res += 2 * S[0] * 3 * U * fro                                                        # the three roundings of X0
    full = dG + 2 * S[0] * np.linalg.norm(ref['bar_X0'])                                 # how far an eigenvalue can move
    sin_t = res / (S[r - 1] ** 2 - s_next ** 2 - 2 * full)
    return dG, bar_S, sin_t


def check_fit(eng, n_points, m, variant, dtype, scale_type, axis_cnt):
    """Sigma_r against the singular values of the longdouble X0, the first three training snapshots reconstructed against
    the rank-r truncation of that X0, unscaled"""
    r = 4 if m == 7 else 6
    X = make_case(n_points, m, variant, dtype)
    spr = SPR(X, F, None, engine=eng)
    if variant == 'signed' and scale_type == 'poisson':
        with pytest.raises(np.linalg.LinAlgError):
            spr.fit(scale_type=scale_type, axis_cnt=axis_cnt, select_modes='number', n_modes=r)
        return spr, {}
    ref, Uu, S, Vt = reference_svd(n_points, m, variant, dtype, scale_type, axis_cnt)
    rows = ref['rows']
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    spr.fit(scale_type=scale_type, axis_cnt=axis_cnt, select_modes='number', n_modes=r)
    dG, bar_S, sin_t = spectrum_bars(ref, S, Vt, n_points, m, axis_cnt, r)
    assert_small('Sigma_r', bar_S / S[:r])
    out = dict(Sigma_r=worst(np.abs(spr.Sigma_r - S[:r]), bar_S))
    field0 = (Uu[:, :r] * S[:r]) @ Vt[:r, :3]                                            # (n, 3), scaled units
    scl, cnt = ref['scl'][rows][:, None], ref['cnt'][:, None]
    want = scl * field0.astype(LD) + cnt
    got = spr.reconstruct(spr.Ar[:3])
    assert got.shape == (F * n_points, 3)
    ascl = np.abs(f64(ref['scl']))[rows]
    xw = f64(ref['st']['x']).reshape(F * n_points, m)
    bar = (sin_t * ascl * np.linalg.norm(f64(ref['X0']), axis=1) + (m + r + 8) * U * np.sqrt(r) * np.linalg.norm(xw, axis=1)
           + ascl * np.linalg.norm(ref['bar_X0'], axis=1) + ref['bar_cnt']
           + ascl * np.max(np.abs(field0), axis=1) * (ref['rel_scl'][rows] + 3 * U) + U * np.max(np.abs(f64(want)), axis=1))
    for f in range(F):
        assert_small('field', np.max(bar[rows == f]) / np.max(np.abs(f64(want[rows == f]))))   # of the feature's largest entry
    out['field'] = worst(np.abs(got - want), bar[:, None])
    print(f'fit {n_points}x{m} {variant} {dtype} {scale_type} axis_cnt={axis_cnt} r={r}: kappa {S[0] / S[r - 1]:.1f} '
          f'error / bar ' + ' '.join(f'{k} {v:.3f}' for k, v in out.items()))
    return spr, out


def device_route_condition(n_points, m, variant, dtype, scale_type):
    """What fit() asks of the data before it stays on its all-device route (m <= 24, row centring, a code scaling): sigma_1 /
    sigma_r <= 1e4 and no centre so large that the projection must pre-centre, with a factor 4 to spare -- a condition on the
    data, from the reference alone"""
    r = 4 if m == 7 else 6
    ref, Uu, S, Vt = reference_svd(n_points, m, variant, dtype, scale_type, 1)
    st = ref['st']
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    fluct = np.sum(f64(st['x'] - st['rowmean'][:, :, None]) ** 2, axis=(1, 2)) / (n_points * m)
    ratio = (np.abs(f64(st['mean'])) + 4 * np.sqrt(np.maximum(f64(st['var']) - fluct, 0.0))) / np.sqrt(fluct)
    kappa = S[0] / S[r - 1]
    return kappa * 4 < 1e4 and ratio.max() * kappa * 4 < 1e6


# ------------------------------------------------------------------------------------------------ the tests of this file
@pytest.fixture(scope='module')
def eng():
    return NumpyEngine()


@pytest.mark.parametrize('variant', ['positive', 'signed'])
@pytest.mark.parametrize('n_points,m', SHAPES + [WIDE])
def test_the_eleven_scalings_are_told_apart(n_points, m, variant):
    """A condition on the data: for every feature, any two of the eleven scale factors differ by at least 1e-3 relative
    (NaN, the signed 'poisson', differs from everything); 'signed' has the signs it promises."""
    for dtype in ('f64', 'f32'):
        st = block_stats(n_points, m, variant, dtype)
        s = np.array([np.asarray(ref_scale(st, t), dtype=np.float64) for t in SCALINGS])     # (11, F)
        for f in range(F):
            for a in range(len(SCALINGS)):
                for b in range(a):
                    if np.isfinite(s[a, f]) and np.isfinite(s[b, f]):
                        gap = abs(s[a, f] - s[b, f]) / max(abs(s[a, f]), abs(s[b, f]))
                        assert gap >= 1e-3, (SCALINGS[a], SCALINGS[b], f, s[a, f], s[b, f])
        x = np.asarray(st['x'], dtype=np.float64)
        if variant == 'positive':
            assert np.all(st['mean'] > 0)
        else:
            assert st['mean'][0] < 0 < x[0].max() and x[0].min() < 0 and x[3].max() < 0 and st['mean'][1] > 0 and st['mean'][2] > 0
            assert np.array_equal(np.isnan(s[SCALINGS.index('poisson')]), [True, False, False, True])
            for t in ('level', 'vast', 'max', 'median'):
                assert s[SCALINGS.index(t), 3] < 0


@pytest.mark.parametrize('variant', ['positive', 'signed'])
@pytest.mark.parametrize('n_points,m', [(77, 7), (77, 24)])
def test_the_data_stays_on_the_all_device_route(n_points, m, variant):
    for scale_type in CODE_SCALINGS:
        if not (variant == 'signed' and scale_type == 'poisson'):
            assert device_route_condition(n_points, m, variant, 'f64', scale_type), scale_type
            assert device_route_condition(n_points, m, variant, 'f32', scale_type), scale_type


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('variant', ['positive', 'signed'])
@pytest.mark.parametrize('scale_type', SCALINGS)
@pytest.mark.parametrize('n_points,m,axis_cnt', CASES, ids=IDS)
def test_restatement_agrees_with_the_oracle(n_points, m, axis_cnt, scale_type, variant, dtype):
    """The longdouble restatement, rounded to float64, against oracle.spr_oracle.scale_data on the widened values: np.std /
    np.average sum pairwise, a few eps times the conditioning of the block mean (A_f / |mu_f|) where a scale derives from it."""
    ref = reference(n_points, m, variant, dtype, scale_type, axis_cnt)
    Xw = make_case(n_points, m, variant, dtype).astype(np.float64)
    with np.errstate(invalid='ignore'):
        X_cnt, X_scl, X0 = orc.scale_data(Xw, F, scale_type, axis_cnt)
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    st, rows, fin = ref['st'], ref['rows'], ref['finite']
    cond = 1.0 + f64(st['A'] / np.abs(st['mean']))
    scl = X_scl[::n_points, 0]
    assert np.array_equal(np.isnan(scl), ~fin)
    assert np.all(np.abs(scl[fin] - ref['scl'][fin]) <= 16 * U * cond[fin] * np.abs(f64(ref['scl'])[fin]))
    assert np.all(np.abs(X_cnt[:, 0] - ref['cnt']) <= 16 * U * (f64(st['rowabs']).reshape(-1) if axis_cnt is not None else f64(st['A'])[rows]))
    rfin = fin[rows]
    assert np.all(np.abs(X0[rfin] - ref['X0'][rfin]) <= ref['bar_X0'][rfin])


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('variant', ['positive', 'signed'])
@pytest.mark.parametrize('scale_type', SCALINGS)
@pytest.mark.parametrize('n_points,m,axis_cnt', CASES, ids=IDS)
def test_scale_data_matrix(eng, n_points, m, axis_cnt, scale_type, variant, dtype):
    check_scale_data(eng, n_points, m, variant, dtype, scale_type, axis_cnt)


@pytest.mark.parametrize('scale_type', SCALINGS)
@pytest.mark.parametrize('axis_cnt', AXES)
def test_scale_data_on_a_column_slice(eng, scale_type, axis_cnt):
    check_scale_data(eng, 130, 65, 'signed', 'f64', scale_type, axis_cnt, wrap=wrap_column_slice(eng.to_device))


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('n_points,m,row0,n_loc', WINDOWS)
def test_kernels_on_row_windows(eng, n_points, m, row0, n_loc, dtype):
    check_kernels_on_window(eng, n_points, m, row0, n_loc, dtype)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('variant', ['positive', 'signed'])
@pytest.mark.parametrize('scale_type', SCALINGS)
@pytest.mark.parametrize('n_points,m,axis_cnt', CASES, ids=IDS)
def test_fit_per_combination(eng, n_points, m, axis_cnt, scale_type, variant, dtype):
    check_fit(eng, n_points, m, variant, dtype, scale_type, axis_cnt)
