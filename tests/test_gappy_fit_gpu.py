"""ROM.fit_gappy on the HIP engine: the row-fill and fill kernels (csrc/gappy_fill.hip) against the NumPy statements of
tests/test_gappy_fit_host.py at the smallest shapes where they can go wrong -- 201 rows (67 points x 3 of 5 features: not a
multiple of 64, feature boundaries inside a panel), m in {1, 13, 20, 70} (70: two 64-column words), r in {1, 7, 64, 128} (every
instantiation; r = 128: the slice of A is 64 columns, so m = 70 takes two slices), all four storage suffixes, row0 in
{0, 134}, strided X and mask -- one long block (more workgroups than one, several panels per wave) and the public method.

Bars: derived in the docstring of tests/test_gappy_fit_host.py; the exact values are formed in np.longdouble there."""
import warnings

import numpy as np
import pytest

from tests.test_gappy_fit_host import (EPS, EPS32, KW3, check_against_numpy_loop, filled_of, low_rank_case, numpy_fill,
                                       numpy_rowfill, rel_hole_error, sums_of)

pytestmark = pytest.mark.gpu
N_POINTS, F_GLOBAL, N_ROWS = 67, 5, 201


@pytest.fixture(scope='module')
def eng():
    from openmeasure_amd.engine import HipEngine
    return HipEngine('cuda:0')


def _mask(rng, n, m, kind):
    """20 % random holes; row 3 with a single observed entry; 'panel': rows 64..127 (one whole panel) without a hole;
    'column': column m - 1 with a single observed row (the two exclude each other)"""
    obs = rng.random((n, m)) >= 0.2
    if m > 1:
        obs[3] = False
        obs[3, m // 2] = True
    if kind == 'panel':
        obs[64:128] = True
    elif m > 1:
        obs[:, m - 1] = False
        obs[150, m - 1] = True
    return obs


def _strided(eng, a, pad, dtype):
    """device view (n, m) of a row-major buffer (n, m + pad) -> (view, buffer)"""
    n, m = a.shape
    buf = np.full((n, m + pad), 77, dtype=a.dtype)
    buf[:, :m] = a
    t = eng.to_device(buf, dtype=dtype)
    return t[:, :m], t


def _inputs(eng, seed, m, r, x32, u32, row0, kind=None):
    import torch
    rng = np.random.default_rng(seed)
    n = N_ROWS
    obs = _mask(rng, n, m, kind or ('panel' if row0 == 0 else 'column'))
    X = rng.standard_normal((n, m)) + 2.0
    U, A = rng.standard_normal((n, r)), rng.standard_normal((m, r))
    mu, scale = rng.standard_normal(n), rng.uniform(0.5, 2.0, F_GLOBAL)
    if x32:
        X = X.astype(np.float32)
    if u32:
        U = U.astype(np.float32)
    Xv, Xbuf = _strided(eng, X, 3, torch.float32 if x32 else torch.float64)
    Mv, _ = _strided(eng, obs.astype(np.uint8) * 5, 5, torch.uint8)          # any non-zero byte means observed
    Ud = eng.to_device(U, dtype=torch.float32 if u32 else torch.float64)
    return dict(obs=obs, X=X, U=U.astype(np.float64), A=A, mu=mu, scale=scale, Xv=Xv, Xbuf=Xbuf, Mv=Mv, Ud=Ud, row0=row0,
                mu_d=eng.to_device(mu), scale_d=eng.to_device(scale), A_d=eng.to_device(A), r=r, m=m, x32=x32)


def _fill(eng, c, Ud=None):
    return eng.to_host(eng.gappy_fill(c['Ud'] if Ud is None else Ud, c['row0'], N_POINTS, F_GLOBAL, c['mu_d'], c['scale_d'],
                                      c['A_d'], c['Xv'], c['Mv'])).copy()


def _check_fill(eng, c, s, X_old):
    got_buf = eng.to_host(c['Xbuf']).copy()
    got = got_buf[:, :c['m']]
    ref = numpy_fill(c['U'], c['row0'], N_POINTS, F_GLOBAL, c['mu'], c['scale'], c['A'], X_old, c['obs'])
    hi, hj = ref['hi'], ref['hj']
    bar = ref['bar'] + (EPS32 * np.abs(ref['new']).astype(np.float64) if c['x32'] else 0.0)
    err = np.abs(got[hi, hj] - ref['new']).astype(np.float64)
    print('fill: holes', len(hi), 'worst err / bar', float((err / bar).max()) if len(hi) else 0.0)
    assert np.all(err <= bar)
    # observed entries and the padding keep their bytes
    assert np.array_equal(got[c['obs']], X_old[c['obs']]) and np.all(got_buf[:, c['m']:] == 77)
    sd, sn = sums_of(got, X_old, hi, hj)
    gam = (len(hi) + c['r'] + 4) * EPS
    print('S_d, S_n rel err / bar', float(abs(s[0] - sd) / (gam * sd)) if sd else 0.0, float(abs(s[1] - sn) / (gam * sn)) if sn else 0.0)
    assert abs(s[0] - sd) <= gam * sd and abs(s[1] - sn) <= gam * sn
    return got


@pytest.mark.parametrize('suffix', ['f64', 'x32', 'u32', 'x32_u32'])
@pytest.mark.parametrize('r', [1, 7, 64, 128])
@pytest.mark.parametrize('m', [1, 13, 20, 70])
def test_fill_kernel_against_numpy(eng, m, r, suffix):
    for row0 in (0, 134):
        c = _inputs(eng, 1000 * m + r, m, r, 'x32' in suffix, 'u32' in suffix, row0)
        s = _fill(eng, c)
        _check_fill(eng, c, s, c['X'])


@pytest.mark.parametrize('x32', [False, True])
@pytest.mark.parametrize('m', [13, 20, 70])
def test_rowfill_kernel_against_numpy(eng, m, x32):
    for row0 in (0, 134):
        c = _inputs(eng, 50 + m, m, 7, x32, False, row0)
        X = c['X'].copy()
        X[~c['obs']] = np.nan                                   # holes may hold anything
        c['Xv'].copy_(eng.to_device(X, dtype=c['Xv'].dtype))
        rec = eng.to_host(eng.gappy_rowfill(c['Xv'], row0, c['Mv']))
        _, want, mean, mabs = numpy_rowfill(X, row0, c['obs'])
        np.testing.assert_array_equal(rec[:5], want)
        assert rec[1] == 0 and rec[3] == 0 and np.all(rec[5:] == 0)
        buf = eng.to_host(c['Xbuf'])
        got = buf[:, :m]
        hi, hj = np.nonzero(~c['obs'])
        bar = (m + 2) * EPS * mabs[hi] + (EPS32 * np.abs(mean[hi]) if x32 else 0.0)
        assert np.all(np.abs(got[hi, hj] - mean[hi]) <= bar)
        assert np.array_equal(got[c['obs']], X[c['obs']]) and np.all(buf[:, m:] == 77)


def test_nan_basis_rows_of_a_panel_without_a_hole_reach_nothing(eng):
    """NaN in the basis rows of a panel without a hole: sums and X are finite and bitwise those of the clean run.  (The
    kernel leaves such a panel before it requests these rows; what this test can show is that they reach no output.)"""
    c = _inputs(eng, 7, 20, 7, False, False, 134, kind='panel')
    s0 = _fill(eng, c)
    want = eng.to_host(c['Xbuf']).copy()
    c['Xv'].copy_(eng.to_device(c['X']))
    Ubad = c['Ud'].clone()
    Ubad[64:128] = float('nan')                                 # rows 64..127: the panel without a hole
    s1 = _fill(eng, c, Ud=Ubad)
    assert np.all(np.isfinite(s1)) and np.array_equal(s0, s1)
    np.testing.assert_array_equal(eng.to_host(c['Xbuf']), want)


def test_nan_in_holes_is_overwritten(eng):
    c = _inputs(eng, 8, 20, 7, False, False, 0)
    X = c['X'].copy()
    X[~c['obs']] = np.nan
    c['Xv'].copy_(eng.to_device(X))
    rec = eng.to_host(eng.gappy_rowfill(c['Xv'], 0, c['Mv']))
    assert rec[0] == (~c['obs']).sum() and rec[1] == 0 and rec[3] == 0
    start = eng.to_host(c['Xbuf'])[:, :20].copy()               # the row-mean fill: what the driver's first pass starts from
    assert np.all(np.isfinite(start))
    s = _fill(eng, c)
    assert np.all(np.isfinite(s))
    got = _check_fill(eng, c, s, start)
    assert np.all(np.isfinite(got))
    # a NaN left in a hole: the hole is overwritten with the finite value, only S_d sees the old one
    c['Xv'].copy_(eng.to_device(X))
    s = _fill(eng, c)
    assert np.isnan(s[0]) and np.isfinite(s[1]) and np.array_equal(eng.to_host(c['Xbuf'])[:, :20], got)


def test_many_panels_and_bitwise_repeat(eng):
    import torch
    rng = np.random.default_rng(11)
    n_points, F, m, r = 22000, 3, 8, 7
    n = n_points * F
    obs = rng.random((n, m)) >= 0.05
    X = rng.standard_normal((n, m)) + 2.0
    U, A = rng.standard_normal((n, r)), rng.standard_normal((m, r))
    mu, scale = rng.standard_normal(n), rng.uniform(0.5, 2.0, F)
    Md = eng.to_device(obs.astype(np.uint8), dtype=torch.uint8)
    Ud, A_d, mu_d, scale_d = eng.to_device(U), eng.to_device(A), eng.to_device(mu), eng.to_device(scale)
    runs = []
    for _ in range(2):
        Xd = eng.to_device(X)
        s = eng.to_host(eng.gappy_fill(Ud, 0, n_points, F, mu_d, scale_d, A_d, Xd, Md)).copy()
        runs.append((s, eng.to_host(Xd).copy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    s, got = runs[0]
    ref = numpy_fill(U, 0, n_points, F, mu, scale, A, X, obs)
    hi, hj = ref['hi'], ref['hj']
    assert np.all(np.abs(got[hi, hj] - ref['new']) <= ref['bar']) and np.array_equal(got[obs], X[obs])
    sd, sn = sums_of(got, X, hi, hj)
    gam = (len(hi) + r + 4) * EPS
    assert abs(s[0] - sd) <= gam * sd and abs(s[1] - sn) <= gam * sn


def test_refusals(eng):
    import torch
    c = _inputs(eng, 9, 13, 7, False, False, 134)
    before = eng.to_host(c['Xbuf']).copy()
    with pytest.raises(NotImplementedError, match='129'):       # SPR_E_UNSUPPORTED
        eng.gappy_fill(eng.zeros((N_ROWS, 129)), 134, N_POINTS, F_GLOBAL, c['mu_d'], c['scale_d'], eng.zeros((13, 129)), c['Xv'],
                       c['Mv'])
    np.testing.assert_array_equal(eng.to_host(c['Xbuf']), before)
    obs = c['obs'].copy()
    obs[[40, 170]] = False                                      # two rows of zeros
    X = c['X'].copy()
    X[~obs] = 1e30
    i, j = np.argwhere(obs)[500]
    X[i, j] = np.nan                                            # a NaN at an observed entry
    Xd, Md = eng.to_device(X), eng.to_device(obs.astype(np.uint8), dtype=torch.uint8)
    rec = eng.to_host(eng.gappy_rowfill(Xd, 134, Md))
    np.testing.assert_array_equal(rec[:5], [(~obs).sum(), 2, 134 + 40, 1, 134 + i])
    np.testing.assert_array_equal(rec[:5], numpy_rowfill(X, 134, obs)[1])
    assert np.array_equal(eng.to_host(Xd), X, equal_nan=True)   # nothing written: not in the bad rows, not anywhere


# ------------------------------------------------------------------------------------------------------ the public method
def test_exact_recovery(eng):
    from openmeasure_amd.sparse_sensing import ROM
    case = low_rank_case(0)
    keep = case['X'].copy()
    rom = ROM(case['X'], case['F'], None, engine=eng)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        rom.fit_gappy(tol=1e-6, max_iter=500, **KW3)
    info = rom.gappy_fit_info_
    got = filled_of(rom)
    err = rel_hole_error(got, case)
    print('fit_gappy (HIP): iterations', info['iterations'], 'rel hole error', err)
    assert info['converged'] and info['iterations'] <= 500 and err <= 1e-3
    assert info['holes'] == (~case['obs']).sum()
    assert np.array_equal(case['X'], keep, equal_nan=True)      # the caller's ndarray is untouched
    np.testing.assert_array_equal(got[case['obs']], keep[case['obs']])


def test_against_the_numpy_loop(eng):
    """the driver and the kernels, hole by hole, against the plain NumPy SVD loop: bar and its accumulation as derived in
    tests/test_gappy_fit_host.py::test_against_the_numpy_loop"""
    from openmeasure_amd.sparse_sensing import ROM
    case = low_rank_case(9)
    rom = ROM(case['X'], case['F'], None, engine=eng)
    with pytest.warns(RuntimeWarning, match='did not converge in 3 fill passes'):
        rom.fit_gappy(max_iter=3, **KW3)
    check_against_numpy_loop(rom, case)


def test_large_block_full_grid_and_grid_stride(eng):
    """1.1M rows x 8: 17 188 panels (the fill kernel's grid is capped at two workgroups per CU and every wave strides over
    several panels) and more rows than one sweep of the row fill's 8 workgroups per CU covers (its grid-stride loop);
    against the longdouble statements at the same bars."""
    import torch
    rng = np.random.default_rng(12)
    n_points, F, m, r = 550_000, 2, 8, 7
    n = n_points * F
    obs = rng.random((n, m)) >= 0.05
    obs[np.arange(n), rng.integers(0, m, n)] = True
    X = rng.standard_normal((n, m)) + 2.0
    U, A = rng.standard_normal((n, r)), rng.standard_normal((m, r))
    mu, scale = rng.standard_normal(n), rng.uniform(0.5, 2.0, F)
    Md = eng.to_device(obs.astype(np.uint8), dtype=torch.uint8)
    Xd = eng.to_device(X)
    s = eng.to_host(eng.gappy_fill(eng.to_device(U), 0, n_points, F, eng.to_device(mu), eng.to_device(scale), eng.to_device(A),
                                   Xd, Md)).copy()
    got = eng.to_host(Xd).copy()
    ref = numpy_fill(U, 0, n_points, F, mu, scale, A, X, obs)
    hi, hj = ref['hi'], ref['hj']
    assert np.all(np.abs(got[hi, hj] - ref['new']) <= ref['bar']) and np.array_equal(got[obs], X[obs])
    sd, sn = sums_of(got, X, hi, hj)
    gam = (len(hi) + r + 4) * EPS
    assert abs(s[0] - sd) <= gam * sd and abs(s[1] - sn) <= gam * sn
    Xd = eng.to_device(X)
    rec = eng.to_host(eng.gappy_rowfill(Xd, 0, Md))
    _, want, mean, mabs = numpy_rowfill(X, 0, obs)
    np.testing.assert_array_equal(rec[:5], want)
    assert rec[0] == len(hi) and rec[1] == 0 and rec[3] == 0
    got = eng.to_host(Xd)
    assert np.all(np.abs(got[hi, hj] - mean[hi]) <= (m + 2) * EPS * mabs[hi]) and np.array_equal(got[obs], X[obs])


def test_end_state_is_a_fit_and_in_place(eng):
    import torch
    from openmeasure_amd.rom import DeviceMatrix
    from openmeasure_amd.sparse_sensing import SPR
    case = low_rank_case(2)
    T = eng.to_device(case['X'])
    spr = SPR(DeviceMatrix(T), case['F'], None, engine=eng)
    with pytest.warns(RuntimeWarning, match='did not converge'):
        spr.fit_gappy(max_iter=3, **KW3)
    assert spr.X.tensor is T and bool(torch.isfinite(T).all())
    filled = eng.to_host(T).copy()
    np.testing.assert_array_equal(filled[case['obs']], case['X'][case['obs']])
    state = [np.array(spr.Ur), np.array(spr.Ar), np.array(spr.X_cnt)]
    spr.fit(**KW3)
    for a, b in zip(state, (spr.Ur, spr.Ar, spr.X_cnt)):
        np.testing.assert_array_equal(a, b)
    C = spr.optimal_placement()
    spr.train(C)
    y = np.zeros((len(spr.sensors_), 3))
    y[:, 0] = filled[spr.sensors_, 0]
    y[:, 2] = spr.sensors_ // case['n_points']
    a, _ = spr.predict(y)
    assert spr.reconstruct(a).shape == (case['X'].shape[0], 1)


def test_two_runs_agree_bit_for_bit(eng):
    from openmeasure_amd.sparse_sensing import ROM
    case = low_rank_case(3)
    out = []
    for _ in range(2):
        rom = ROM(case['X'], case['F'], None, engine=eng)
        with pytest.warns(RuntimeWarning):
            rom.fit_gappy(max_iter=4, **KW3)
        out.append((filled_of(rom).copy(), rom.gappy_fit_info_, np.array(rom.Ar)))
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1] and np.array_equal(out[0][2], out[1][2])
    # an explicit device-tensor mask over garbage in the holes = mask=None on NaN-coded data
    import torch
    rom = ROM(np.where(case['obs'], case['X'], 1e30), case['F'], None, engine=eng)
    with pytest.warns(RuntimeWarning):
        rom.fit_gappy(eng.to_device(case['obs'].astype(np.uint8), dtype=torch.uint8), max_iter=4, **KW3)
    assert np.array_equal(filled_of(rom), out[0][0]) and rom.gappy_fit_info_ == out[0][1]
