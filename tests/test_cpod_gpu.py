"""ROM.CPOD on the HIP engine: the batched bound sweep (spr_bound_sweep_batch_*, csrc/bounds.hip) against the contract
numpy_bound_sweep states (tests/test_cols_host.py) and against the existing 16-vector sweep, and the whole
fit -> CPOD chain against the KKT conditions of the full problem.  Yardsticks, derivations and bars are those of
tests/test_cpod_host.py (measured there on the CPU loop; the HIP path is held to the same STAT_BAR 1.7e-15, COMP_BAR 3.1e-15)."""
import numpy as np
import pytest

from tests.test_cols_gpu import _sweep_case
from tests.test_cols_host import _feas_round, make_case, scaled_limits
from tests.test_cpod_host import CASES, fitted, kkt_all, same_bar

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    from openmeasure_amd.engine import HipEngine
    return HipEngine('cuda:0')


def _args(eng, c):
    return (c['Ud'], c['row0'], c['n_points'], c['F'], eng.to_device(c['mu']), eng.to_device(c['scale']),
            eng.to_device(c['limits']), eng.to_device(c['clamp']), eng.to_device(c['G']))


SHAPES = [(6, 1, 0, False), (6, 100, 2, True), (32, 16, 0, False), (32, 256, 0, True), (64, 17, 0, True), (64, 64, 8, False),
          (64, 256, 0, False), (100, 64, 0, False), (100, 17, 6, True), (128, 100, 0, True), (128, 256, 0, False),
          (128, 1, 2, False), (200, 16, 0, False), (200, 100, 6, True), (7, 17, 0, False)]


def _check_against_numpy(eng, c, n_p, tag):
    """bound_sweep_batch on the case c against the contract numpy_bound_sweep states and against bound_sweep"""
    tol, k = 0.05, 24
    args = _args(eng, c)
    out = eng.to_host(eng.bound_sweep_batch(*args, tol, k))
    again = eng.to_host(eng.bound_sweep_batch(*args, tol, k))
    old = eng.to_host(eng.bound_sweep(*args, tol, k))
    assert out.shape == (n_p, 3 + 3 * k)
    assert np.array_equal(out, again)                             # no atomics: two runs are bit-identical
    lo0, hi0, feat = scaled_limits(c['row0'], c['n'], c['n_points'], c['F'], c['mu'], c['scale'], c['limits'], c['clamp'])
    worst_margin = np.inf
    rnd_unit = _feas_round(c['U'], np.eye(1, c['U'].shape[1])[0])  # _feas_round is linear in |g|: one pass over U for all p
    for p in range(n_p):
        g = c['G'][p]
        x = c['U'] @ g
        v2 = np.stack([lo0 - x, x - hi0], axis=1)
        v = v2.max(axis=1)
        rnd = rnd_unit * np.linalg.norm(g)                        # two summation orders of the same dot product
        # the seeded inputs leave no row within rnd of tol or of the runner-up: count and row are then determined
        top = np.partition(v, -2)[-2:]
        margin = min(np.abs(v2 - tol).min(), top[1] - top[0])
        worst_margin = min(worst_margin, margin / rnd)
        assert margin > 2 * rnd, (p, margin, rnd)
        assert abs(out[p, 0] - v.max()) <= rnd
        assert int(out[p, 1]) == c['row0'] + int(np.argmax(v))
        assert int(out[p, 2]) == np.count_nonzero(v > tol)
        # the first three fields against the existing sweep
        assert abs(out[p, 0] - old[p, 0]) <= rnd and out[p, 1] == old[p, 1] and out[p, 2] == old[p, 2]
        cand = out[p, 3:].reshape(k, 3)
        used = cand[cand[:, 0] >= 0]
        assert np.all(cand[len(used):, 0] == -1) and np.all(np.isneginf(cand[len(used):, 2]))
        if v.max() <= tol:
            assert len(used) == 0
            continue
        assert int(used[0, 0]) == int(out[p, 1]) and used[0, 2] == out[p, 0]      # the global worst is the first candidate
        assert np.all(np.diff(used[:, 2]) <= 0)                                  # worst first
        keys = set()
        for rw, side, val in used:
            i, sd = int(rw) - c['row0'], int(side)
            assert 0 <= i < c['n'] and sd in (0, 1) and (i, sd) not in keys
            keys.add((i, sd))
            assert abs(v2[i, sd] - val) <= rnd and val > tol                    # every candidate is really violated
    print('batch sweep', tag, 'smallest margin / rounding', worst_margin)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('r,n_p,ldu_pad,clamped', SHAPES)
def test_bound_sweep_batch_against_numpy(eng, dtype, r, n_p, ldu_pad, clamped):
    """the block of _sweep_case starts inside feature 1 of 4 and ends inside feature 3; n is no multiple of any tile.
    With 2 863 rows every workgroup gets ONE 64-row panel; the steady-state loop is test_..._many_panels below."""
    c = _sweep_case(eng, r, n_p, dtype, seed=300 + r + n_p, ldu_pad=ldu_pad, clamp_feature=clamped)
    assert c['Ud'].stride(0) == r + ldu_pad
    _check_against_numpy(eng, c, n_p, (dtype, r, n_p))


def _long_case(eng, r, n_p, dtype, seed, ldu_pad, clamp_feature):
    """_sweep_case with features of 100 003 cells: the block (238 909 rows) starts inside feature 1 of 4 and ends inside
    feature 3, no boundary and no length is a multiple of 64"""
    import torch
    rng = np.random.default_rng(seed)
    n_points, F = 100_003, 4
    row0, n = n_points + 33_217, 2 * n_points + 38_903
    U = (rng.standard_normal((n, r)) / np.sqrt(r)).astype(np.float32 if dtype == 'f32' else np.float64)
    Upad = np.zeros((n, r + ldu_pad), dtype=U.dtype)
    Upad[:, :r] = U
    Ud = eng.to_device(Upad, dtype=torch.float32 if dtype == 'f32' else torch.float64)[:, :r]
    mu = rng.standard_normal(n) * 0.3
    scale = rng.uniform(0.5, 2.0, F)
    G = rng.standard_normal((n_p, r))
    limits = np.stack([-rng.uniform(1.0, 2.5, F), rng.uniform(1.0, 2.5, F)])
    clamp = np.full((2, F), np.nan)
    if clamp_feature:
        clamp[1, 2], clamp[0, 1] = 1000.0, -1000.0
    return dict(U=U.astype(np.float64), Ud=Ud, mu=mu, scale=scale, G=G, limits=limits, clamp=clamp, row0=row0, n=n,
                n_points=n_points, F=F)


# r = 32: two workgroups per CU; 64, 100, 128: one.  n_p = 100: both halves of the waves and a partial 16-vector group in the
# second pass; 256: four full passes; 17: one vector in the second group
LONG = [(32, 100, 'f64', 0, False), (32, 17, 'f32', 2, True), (64, 100, 'f64', 0, True), (64, 256, 'f32', 0, False),
        (100, 100, 'f32', 6, True), (128, 100, 'f64', 0, False)]


@pytest.mark.parametrize('r,n_p,dtype,ldu_pad,clamped', LONG)
def test_bound_sweep_batch_many_panels(eng, r, n_p, dtype, ldu_pad, clamped):
    """the steady-state loop of bound_sweep_batch_kernel: every workgroup walks a run of SEVERAL 64-row panels (the single LDS
    panel image is overwritten behind the first barrier, the next panel's registers are handed over, row offsets inside the
    run exceed 63, runs start at c > 0 and the last run of a feature ends in a partial panel).  The launch deals at most
    2 x CUs workgroups over the block, each feature getting its share, so a block of more than 4 x 64 x 2 x CUs rows gives
    every workgroup at least four panels -- asserted from the device's CU count, not assumed."""
    import torch
    c = _long_case(eng, r, n_p, dtype, seed=700 + r + n_p, ldu_pad=ldu_pad, clamp_feature=clamped)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert c['n'] >= 4 * 64 * 2 * cus and c['n'] % 64 and c['row0'] % 64 and c['n_points'] % 64
    assert c['Ud'].stride(0) == r + ldu_pad
    _check_against_numpy(eng, c, n_p, ('long', dtype, r, n_p))


def test_bound_sweep_batch_records_merge_and_validate(eng):
    from openmeasure_amd._cols import merge_records
    c = _sweep_case(eng, 12, 70, 'f64', seed=5)
    args = _args(eng, c)
    a = eng.to_host(eng.bound_sweep_batch(*args, 0.01, 8))
    merged = merge_records(a[None], 8)
    for p, (v, row, count, cands) in enumerate(merged):
        assert v == a[p, 0] and row == int(a[p, 1]) and count == int(a[p, 2])
        assert [c_[0] for c_ in cands] == [int(x) for x in a[p, 3::3] if x >= 0]
    with pytest.raises(ValueError):
        eng.bound_sweep_batch(*args, 0.01, 0)
    with pytest.raises(ValueError):
        eng.bound_sweep_batch(*args, 0.01, 257)
    with pytest.raises(ValueError):
        eng.bound_sweep_batch(*args, -1.0, 8)


@pytest.mark.parametrize('name', sorted(CASES))
def test_cpod_end_to_end_batch_and_fallback(eng, name, monkeypatch):
    import openmeasure_amd._cpod as cpod
    monkeypatch.setattr(cpod, 'BATCH_FROM', 1)                   # every round through the batched kernel, whatever m
    case = make_case(**CASES[name])
    m = case['X'].shape[1]
    rom = fitted(case, engine=eng)
    Ar0, S0 = np.array(rom.Ar), np.array(rom.Sigma_r)
    rom.CPOD({'limits': case['limits']}, solver='CLARABEL')
    info = rom.cpod_info_
    assert info['status'] == ['optimal'] * m and 'X0' not in rom._host
    np.testing.assert_array_equal(rom.Vr, rom.Ar / S0)
    np.testing.assert_array_equal(rom.Sigma_r, S0)
    kkt_all(rom, Ar0, case['limits'], tag='CPOD batch')
    batch = rom.Ar.copy()
    bar = same_bar(rom, Ar0)
    rom.CPOD({'limits': case['limits']})
    np.testing.assert_array_equal(rom.Ar, batch)                  # a second call gives the same Ar

    class NoBatch:                                                # the same engine without the batched sweep: the fallback
        def __init__(self, e):
            self._e = e

        def __getattr__(self, key):
            if key == 'bound_sweep_batch':
                raise AttributeError(key)
            return getattr(self._e, key)
    rom2 = fitted(case, engine=NoBatch(eng))
    np.testing.assert_array_equal(np.array(rom2.Ar), Ar0)
    rom2.CPOD({'limits': case['limits']})
    assert rom2.cpod_info_['status'] == ['optimal'] * m
    kkt_all(rom2, Ar0, case['limits'], tag='CPOD fallback')
    diff = np.abs(rom2.Ar - batch).max()
    print('CPOD batch - fallback', name, diff, 'bar', bar)
    assert diff <= bar


def test_cpod_semantics_on_the_device(eng):
    case = make_case(**CASES['c1'])
    m = case['X'].shape[1]
    rom = fitted(case, engine=eng)
    Ar0 = np.array(rom.Ar)
    rom.CPOD({'limits': [case['limits'][0] - 50.0, case['limits'][1] + 50.0]})
    assert rom.cpod_info_['status'] == ['ols'] * m and rom.cpod_info_['sweeps'] == 1
    np.testing.assert_array_equal(rom.Ar, Ar0)
    bad = [case['limits'][0].copy(), case['limits'][1].copy()]
    bad[0][1], bad[1][1] = bad[1][1], bad[0][1]
    rom.CPOD({'limits': bad})
    assert rom.cpod_info_['status'] == ['infeasible'] * m and np.all(np.isnan(rom.Ar))
    with pytest.raises(NotImplementedError):
        rom.CPOD({})
    # clamp path
    case = make_case(seed=9, n_points=500, F=3, m=30, r=8, offset=3.0)
    rom = fitted(case, engine=eng)
    lim = [case['limits'][0].copy(), case['limits'][1].copy()]
    lim[1][1] += 5000.0 * rom._scl_f[1]
    lim[0][2] -= 5000.0 * rom._scl_f[2]
    Ar0 = np.array(rom.Ar)
    rom.CPOD({'limits': lim})
    kkt_all(rom, Ar0, lim, tag='CPOD clamp')
    # f32-stored basis: refused
    import torch
    from openmeasure_amd.rom import DeviceMatrix
    from openmeasure_amd.sparse_sensing import ROM
    X32 = eng.to_device(case['X'].astype(np.float32), dtype=torch.float32)
    r32 = ROM(DeviceMatrix(X32, basis='f32'), case['F'], None, engine=eng)
    r32.fit(select_modes='number', n_modes=case['r'])
    with pytest.raises(NotImplementedError, match='float32'):
        r32.CPOD({'limits': case['limits']})
